"""Case tables for the wave primitives, the fast math and the tree solve of csrc/gq_device.h and csrc/gq_step_kernel.h, with numpy float64
references, and the checks that hold a backend to them.  One table, two backends (the precedent is tests/camera_caster.py): the probe library
on the GPU (tests/device_probe, tests/test_gpu_device_probe.py) and the host emulator's shim (tests/simt_emu, tests/test_device_cases_emulated.py).
TEST INFRASTRUCTURE.

Every bound is the function's own contract (its header comment) or is derived here from the number formats; none comes from a measurement.
Each check returns report rows (name, cases, worst error, bound, unit, worst argument) and asserts after it has measured."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

U24, U23, U22 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22
XOR_MASKS = (1, 2, 4, 8, 16, 32, 17, 63)
READLANES = (0, 15, 31, 47, 63)


class Out:
    """an output argument: allocated (zeroed) by the backend, returned as a numpy array"""
    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, np.dtype(dtype)


_SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


class Backend:
    """Calls `<prefix><fn>` of a C library: numpy arrays go in (host memory, or copied to `device` through torch), Out()s come back as numpy arrays,
    ints and floats are passed by value.  The entry points return a HIP error code (0 on the host)."""
    def __init__(self, lib, prefix, device=None):
        self.lib, self.prefix, self.device = lib, prefix, device

    @property
    def on_device(self):
        return self.device is not None

    def run(self, fn, *args):
        f = getattr(self.lib, self.prefix + fn)
        f.restype = C.c_int
        cargs, outs, keep = [], [], []
        if self.on_device:
            import torch
        for a in args:
            if isinstance(a, Out) or isinstance(a, np.ndarray):
                host = np.zeros(a.shape, a.dtype) if isinstance(a, Out) else np.ascontiguousarray(a)
                if self.on_device:   # torch has no arithmetic on unsigned words: they travel as their signed views
                    t = torch.from_numpy(host.view(_SIGNED.get(host.dtype, host.dtype))).to(self.device)
                    keep.append(t)
                    cargs.append(C.c_void_p(t.data_ptr() if t.numel() else 0))
                    if isinstance(a, Out):
                        outs.append((t, host.dtype))
                else:
                    keep.append(host)
                    cargs.append(C.c_void_p(host.ctypes.data))
                    if isinstance(a, Out):
                        outs.append((host, host.dtype))
            elif isinstance(a, float):
                cargs.append(C.c_float(a))
            else:
                cargs.append(C.c_int(int(a)))
        if self.on_device:
            torch.cuda.synchronize()   # the uploads are done; the entry point launches on the null stream and synchronises itself
        rc = f(*cargs)
        assert rc == 0, f'{self.prefix}{fn}: error code {rc}'
        res = [(t.cpu().numpy() if self.on_device else t).view(dt) for t, dt in outs]
        return res[0] if len(res) == 1 else res


def row(name, n, err, bound, unit, worst=''):
    return dict(name=name, n=int(n), err=float(err), bound=float(bound), unit=unit, worst=str(worst))


def fmt_rows(rows):
    return [f"{r['name']:<28s} cases {r['n']:>7d}   max error {r['err']:.4g} {r['unit']}   bound {r['bound']:.4g} {r['unit']}   worst at {r['worst']}" for r in rows]


def _ulp32(ref):
    """the spacing of float32 at |ref| (float64 in, float64 out)"""
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def _worst(err, bound):
    """index of the case closest to (or farthest beyond) its bound"""
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return int(np.argmax(q))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------- A. wave primitives
@functools.lru_cache(None)
def wave_patterns():
    """dict(f=[npat][64] float32 patterns, kind=[npat] labels): 'int' patterns sum exactly in any order, 'real' do not, 'special' hold
    infinities and signed zeros (min / max only)"""
    rng = np.random.default_rng(2024)
    P, K = [], []

    def add(p, kind):
        P.append(np.asarray(p, dtype=np.float32)); K.append(kind)
    for s in (1000.0, -1000.0):   # one-hots in every lane: the row borders 0, 15, 16, 31, 32, 47, 48, 63 among them
        for l in range(64):
            v = np.zeros(64); v[l] = s; add(v, 'int')
    add(np.arange(64), 'int'); add(np.arange(64)[::-1], 'int'); add(np.arange(64) - 31, 'int'); add(31 - np.arange(64), 'int')
    add((-1.0) ** np.arange(64), 'int'); add(-((-1.0) ** np.arange(64)) * 3, 'int')
    for c in (0.0, 1.0, -7.0, 1024.0):
        add(np.full(64, c), 'int')
    for _ in range(80):
        add(rng.integers(-1024, 1025, 64), 'int')
    for _ in range(60):
        add(rng.normal(0, 1, 64) * 10.0 ** rng.uniform(-3, 3), 'real')
    for _ in range(12):
        add(rng.uniform(0.5, 1.5, 64), 'real')   # same sign: the sum's bound is tight
    for l in (0, 15, 16, 31, 32, 47, 48, 63, 5, 40):
        for s in (np.inf, -np.inf):
            v = rng.normal(0, 1, 64); v[l] = s; add(v, 'special')
    v = np.zeros(64); v[17] = -0.0; add(v, 'special')
    v = np.full(64, -0.0); v[48] = 0.0; add(v, 'special')
    v = rng.uniform(1, 2, 64); v[31] = -0.0; v[32] = 0.0; add(v, 'special')
    return dict(f=np.stack(P), kind=np.array(K))


def check_wave_reduce(be):
    T = wave_patterns()
    f, kind = T['f'], T['kind']
    npat = len(f)
    o = Out(f.shape, np.float32)
    s, mn, mx, qs = be.run('wave_reduce', f, npat, o, o, o, o)
    f64 = np.where((kind == 'special')[:, None] & ~np.isfinite(f), 0.0, f.astype(np.float64))   # for the sums only (the special patterns are not summed)
    fmn, fmx = f.astype(np.float64).min(1, keepdims=True), f.astype(np.float64).max(1, keepdims=True)
    rows = []
    # min / max: exact on every pattern, the same value in all 64 lanes (compared as numbers: the minimum of +0 and -0 may be either zero)
    bad_mn = np.nonzero((mn.astype(np.float64) != fmn).any(1))[0]
    bad_mx = np.nonzero((mx.astype(np.float64) != fmx).any(1))[0]
    rows.append(row('wave_min', npat, len(bad_mn), 0, 'patterns off', bad_mn[:4]))
    rows.append(row('wave_max', npat, len(bad_mx), 0, 'patterns off', bad_mx[:4]))
    # sums: the special patterns (inf - inf) are left out
    fin = kind != 'special'
    ints, real = kind == 'int', kind == 'real'
    ref = f64.sum(1, keepdims=True)
    refq = f64.reshape(npat, 16, 4).sum(2).repeat(4, axis=1)
    bad_s = np.nonzero(ints & (s.astype(np.float64) != ref).any(1))[0]
    bad_q = np.nonzero(ints & (qs.astype(np.float64) != refq).any(1))[0]
    rows.append(row('wave_sum (integers)', ints.sum(), len(bad_s), 0, 'patterns off', bad_s[:4]))
    rows.append(row('quad_sum (integers)', ints.sum(), len(bad_q), 0, 'patterns off', bad_q[:4]))
    # reals: a depth-6 tree on the device, 63 sequential additions in the shim; first-order bound depth * 2^-24 * sum |v|
    depth = 6 if be.on_device else 63
    bnd = depth * U24 * np.abs(f64).sum(1)
    err = np.where(fin, np.abs(np.where(fin[:, None], s.astype(np.float64), 0) - ref).max(1), 0)
    w = _worst(np.where(real, err, 0), bnd)
    rows.append(row('wave_sum (reals)', real.sum(), (err[real] / bnd[real]).max(), 1.0, f'x {depth}*2^-24*sum|v|', f'pattern {w}'))
    bq = 2 * U24 * np.abs(f64).reshape(npat, 16, 4).sum(2).repeat(4, axis=1)   # two additions deep on the device, three in the shim
    bq = bq * (1.0 if be.on_device else 1.5)
    eq = np.abs(np.where(fin[:, None], qs.astype(np.float64), 0) - refq)
    rq = np.where(real[:, None], eq / np.maximum(bq, 1e-300), 0)
    rows.append(row('quad_sum (reals)', real.sum(), rq.max(), 1.0, 'x depth*2^-24*sum|v|', f'pattern {int(rq.max(1).argmax())}'))
    assert len(bad_mn) == 0, ('wave_min', bad_mn, mn[bad_mn[0]], f[bad_mn[0]].min())
    assert len(bad_mx) == 0, ('wave_max', bad_mx, mx[bad_mx[0]], f[bad_mx[0]].max())
    assert (s[fin] == s[fin][:, :1]).all(), 'wave_sum differs between lanes'
    assert len(bad_s) == 0, ('wave_sum', bad_s, s[bad_s[0], 0], ref[bad_s[0]])
    assert len(bad_q) == 0, ('quad_sum', bad_q)
    assert (err[real] <= bnd[real]).all(), ('wave_sum reals', w, err[w], bnd[w])
    assert (rq <= 1.0).all(), 'quad_sum reals'
    return rows


def check_wave_scan(be):
    rng = np.random.default_rng(7)
    P = [np.eye(64, dtype=np.int32)[l] * 1000 for l in range(64)] + [np.ones(64, np.int32), np.arange(64, dtype=np.int32)]
    P += [rng.integers(-1000, 1001, 64).astype(np.int32) for _ in range(62)]
    P = np.stack(P).astype(np.int32)
    got = be.run('wave_scan', P, len(P), Out(P.shape, np.int32))
    bad = np.nonzero((got != np.cumsum(P, axis=1)).any(1))[0]
    assert len(bad) == 0, ('wave_incl_scan', bad, got[bad[0]], np.cumsum(P[bad[0]]))
    return [row('wave_incl_scan', len(P), 0, 0, 'patterns off')]


def check_lane_moves(be):
    """bcast from every lane, readlane<0, 15, 31, 47, 63>, shfl_xor for eight masks, shfl_idx for eight permutations: bit for bit"""
    rng = np.random.default_rng(11)
    rows = []
    v = rng.normal(0, 1, (64, 64)).astype(np.float32)
    v[3, 10] = -0.0; v[5, 63] = np.inf   # moved as bits
    src = np.arange(64, dtype=np.int32)
    o = Out(v.shape, np.float32)
    bf, bi = be.run('bcast', v, src, 64, o, Out(v.shape, np.int32))
    want = _bits(v)[np.arange(64), src][:, None].repeat(64, 1)
    assert np.array_equal(_bits(bf), want) and np.array_equal(bi.view(np.uint32), want), 'bcast'
    rows.append(row('bcast (float, int)', 64, 0, 0, 'sources off'))
    rl = be.run('readlane', v[:8], 8, Out((8, 5, 64), np.float32))
    for k, l in enumerate(READLANES):
        assert np.array_equal(_bits(rl[:, k]), _bits(v[:8, l])[:, None].repeat(64, 1)), ('readlane', l)
    rows.append(row('readlane<0,15,31,47,63>', 8 * 5, 0, 0, 'lanes off'))
    xf, xi = be.run('shfl_xor', v[:8], 8, Out((8, 8, 64), np.float32), Out((8, 8, 64), np.int32))
    for k, m in enumerate(XOR_MASKS):
        want = _bits(v[:8])[:, np.arange(64) ^ m]
        assert np.array_equal(_bits(xf[:, k]), want) and np.array_equal(xi[:, k].view(np.uint32), want), ('shfl_xor', m)
    rows.append(row('shfl_xor (8 masks)', 8 * 8, 0, 0, 'masks off'))
    idx = np.stack([rng.permutation(64) for _ in range(8)]).astype(np.int32)
    sf, si = be.run('shfl_idx', v[:8], idx, 8, Out((8, 64), np.float32), Out((8, 64), np.int32))
    want = np.take_along_axis(_bits(v[:8]), idx.astype(np.int64), axis=1)
    assert np.array_equal(_bits(sf), want) and np.array_equal(si.view(np.uint32), want), 'shfl_idx'
    rows.append(row('shfl_idx (8 permutations)', 8, 0, 0, 'permutations off'))
    return rows


def _popc(m):
    return np.array([bin(int(x)).count('1') for x in m.ravel()], np.int32).reshape(m.shape)


def _ffs(m):
    return np.array([(int(x) & -int(x)).bit_length() - 1 for x in m.ravel()], np.int32).reshape(m.shape)


def check_ballot_bits(be):
    """ballot (all zero, all one, every single lane, random), popc64 and ffs64 of the result; popc64 / ffs64 per lane on single bits and random
    masks.  ffs64(0) is -1 on the device (__ffsll); the shim's __builtin_ctzll(0) is undefined and no caller passes 0 (every call site tests
    its mask first or takes the ballot of `value == wave_min / wave_max of the values`, which at least one lane satisfies), so the host run
    leaves the empty mask out."""
    rng = np.random.default_rng(5)
    P = [np.ones(64, np.int32)] + [np.eye(64, dtype=np.int32)[l] for l in range(64)] + [(rng.random(64) < p).astype(np.int32) for p in (0.02, 0.1, 0.5, 0.9) for _ in range(8)]
    P = [p for p in P if p.any()]
    if be.on_device:
        P.append(np.zeros(64, np.int32))
    P = np.stack(P).astype(np.int32) * np.int32(5)   # any non-zero word is true
    o = Out(P.shape, np.int32)
    mask, pc, fs = be.run('ballot', P, len(P), Out(P.shape, np.uint64), o, o)
    want = np.array([sum(1 << l for l in range(64) if p[l]) for p in P], dtype=np.uint64)[:, None].repeat(64, 1)
    assert np.array_equal(mask, want), 'ballot'
    assert np.array_equal(pc, _popc(want)) and np.array_equal(fs, _ffs(want)), 'popc64 / ffs64 of a ballot'
    m = [np.uint64(1) << np.uint64(b) for b in range(64)] + list(rng.integers(0, 1 << 63, 192, dtype=np.uint64) << np.uint64(1) >> rng.integers(0, 64, 192).astype(np.uint64))
    m += [np.uint64(0xffffffffffffffff), np.uint64(1 << 63), np.uint64(0xffffffff00000000), np.uint64(0x100000000)]
    m = np.array([x for x in m if x != 0] + ([np.uint64(0)] if be.on_device else []), dtype=np.uint64)
    o = Out(m.shape, np.int32)
    pc2, fs2 = be.run('bits', m, len(m), o, o)
    assert np.array_equal(pc2, _popc(m)), 'popc64'
    assert np.array_equal(fs2, _ffs(m)), ('ffs64', m[fs2 != _ffs(m)][:4])
    return [row('ballot', len(P), 0, 0, 'masks off'), row('popc64', len(m) + len(P), 0, 0, 'off'),
            row('ffs64' + (' (0 -> -1 included)' if be.on_device else ''), len(m) + len(P), 0, 0, 'off')]


# ----------------------------------------------------------------------------------------------------------------- B. scalar math
def _pow2_neighbours(lo=-90, hi=90):
    p = (2.0 ** np.arange(lo, hi + 1)).astype(np.float32)
    return np.concatenate([p, np.nextafter(p, np.float32(0)), np.nextafter(p, np.float32(np.inf))])


def _ulp_rows(name, x, got, ref, bound_ulp, arg):
    err = np.abs(got.astype(np.float64) - ref) / _ulp32(ref)
    w = int(err.argmax())
    return row(name, len(x), err[w], bound_ulp, 'ulp', arg(w)), err


def check_unary(be):
    """fast_rcp, fast_sqrt, fast_rsqrt <= 1 ulp (v_rcp_f32 / v_sqrt_f32 / v_rsq_f32) over [1e-30, 1e30] and the powers of two +- 1 ulp;
    fast_cos_turns: |error| <= 1e-6 on [0, 1) (its header comment)"""
    rng = np.random.default_rng(3)
    x = np.concatenate([10.0 ** rng.uniform(-30, 30, 4096), _pow2_neighbours(), [1e-30, 1e30, 1.0, 3.0]]).astype(np.float32)
    t = np.concatenate([rng.random(4096), np.arange(0, 64) / 64.0, np.nextafter(np.arange(1, 65, dtype=np.float32) / 64, np.float32(0)), [0.0, 1e-8, 1e-4]]).astype(np.float32)
    t = t[t < 1.0]
    n = max(len(x), len(t))
    xa = np.concatenate([x, np.ones(n - len(x), np.float32)]); ta = np.concatenate([t, np.zeros(n - len(t), np.float32)])
    ox = be.run('unary', xa, n, Out((4, n), np.float32))
    ot = be.run('unary', ta, n, Out((4, n), np.float32))
    x64 = x.astype(np.float64)
    rows, fails = [], []
    for k, (name, ref) in enumerate((('fast_rcp', 1 / x64), ('fast_sqrt', np.sqrt(x64)), ('fast_rsqrt', 1 / np.sqrt(x64)))):
        r, err = _ulp_rows(name, x, ox[k, :len(x)], ref, 1.0, lambda w: f'x = {x[w]!r}')
        rows.append(r)
        if err.max() > 1.0:
            fails.append(r)
    ec = np.abs(ot[3, :len(t)].astype(np.float64) - np.cos(2 * np.pi * t.astype(np.float64)))
    w = int(ec.argmax())
    rows.append(row('fast_cos_turns', len(t), ec[w], 1e-6, 'abs', f'x = {t[w]!r}'))
    assert not fails and ec[w] <= 1e-6, (fails, rows[-1])
    return rows


def check_fdiv(be):
    """fdiv(a, b) = a * v_rcp_f32(b) <= 2 ulp: divisors over [1e-30, 1e30] and at the powers of two +- 1 ulp with quotients of 1e-6 .. 1e6, and
    the guarded epsilons the kernels divide by (fmaxf(eps, .) with eps = 1e-30 .. 1e-9 in csrc/) under numerators of their own scale and of 1"""
    rng = np.random.default_rng(4)
    b = np.concatenate([10.0 ** rng.uniform(-30, 30, 4096), _pow2_neighbours()]).astype(np.float32)
    a = (b.astype(np.float64) * 10.0 ** rng.uniform(-6, 6, len(b))).astype(np.float32)
    eps = np.array([1e-30, 1e-24, 1e-20, 1e-15, 1e-12, 1e-9], np.float32)
    for num in (lambda e: e, lambda e: 3 * e, lambda e: 0.37 * e, lambda e: np.ones_like(e), lambda e: np.full_like(e, 1e-3)):
        b = np.concatenate([b, eps]); a = np.concatenate([a, num(eps).astype(np.float32)])
    got = be.run('fdiv', a, b, len(a), Out(a.shape, np.float32))
    r, err = _ulp_rows('fdiv', a, got, a.astype(np.float64) / b.astype(np.float64), 2.0, lambda w: f'{a[w]!r} / {b[w]!r}')
    assert err.max() <= 2.0, r
    return [r]


def check_med3(be):
    rng = np.random.default_rng(6)
    lo = rng.normal(0, 1, 512); hi = lo + np.abs(rng.normal(0, 1, 512)); hi[::8] = lo[::8]   # lo == hi among them
    x = rng.normal(0, 2, 512)
    x[1::8] = lo[1::8]; x[2::8] = hi[2::8]; x[3::16] = np.nextafter(lo[3::16].astype(np.float32), np.float32(-np.inf)); x[4::16] = np.nextafter(hi[4::16].astype(np.float32), np.float32(np.inf))
    x, lo, hi = (np.asarray(v, np.float32) for v in (x, lo, hi))
    got = be.run('med3', x, lo, hi, len(x), Out(x.shape, np.float32))
    bad = np.nonzero(got != np.minimum(np.maximum(x, lo), hi))[0]
    assert len(bad) == 0, ('med3', x[bad[:4]], lo[bad[:4]], hi[bad[:4]], got[bad[:4]])
    return [row('med3', len(x), 0, 0, 'off')]


ATAN2_BOUND = 1.2e-7 + 3 * U22   # the polynomial's stated error + 3 ulp of pi (the octant constants and the final subtractions) = 8.4e-7 rad


def check_atan2(be):
    """atan2_fast against arctan2, the difference wrapped to (-pi, pi] ((-0, x < 0) gives +pi where arctan2 gives -pi); (0, 0) gives 0"""
    rng = np.random.default_rng(8)
    th = np.arange(4096) * (2 * np.pi / 4096)
    Y, X = [np.sin(th)], [np.cos(th)]
    for k in range(8):   # the octant borders, +- 1 ulp on either coordinate
        c, s = np.float32(np.cos(k * np.pi / 4)), np.float32(np.sin(k * np.pi / 4))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                Y.append([np.nextafter(s, np.float32(dy * 4)) if dy else s]); X.append([np.nextafter(c, np.float32(dx * 4)) if dx else c])
    m = 10.0 ** rng.uniform(-6, 0, 512)
    sg = rng.choice([-1.0, 1.0], (2, 512))
    Y.append(m * sg[0]); X.append(m * sg[1])                                     # |y| == |x|
    tiny = np.array([1e-30, 1e-20, 1e-10, 1e-38, 0.0, -0.0])
    for sx in (1.0, -1.0):
        Y.append(tiny); X.append(np.full(6, sx)); Y.append(-tiny); X.append(np.full(6, sx))
        X.append(tiny); Y.append(np.full(6, sx)); X.append(-tiny); Y.append(np.full(6, sx))
    a = rng.uniform(-np.pi, np.pi, 2048); mm = 10.0 ** rng.uniform(-6, 0, 2048)
    Y.append(mm * np.sin(a)); X.append(mm * np.cos(a))                           # rotation-matrix entries of every magnitude
    y, x = (np.concatenate([np.asarray(v, np.float64).ravel() for v in V]).astype(np.float32) for V in (Y, X))
    got = be.run('atan2', y, x, len(y), Out(y.shape, np.float32)).astype(np.float64)
    zy = np.array([0.0, 0.0, -0.0, -0.0], np.float32); zx = np.array([0.0, -0.0, 0.0, -0.0], np.float32)
    assert (be.run('atan2', zy, zx, 4, Out((4,), np.float32)) == 0).all(), 'atan2_fast(0, 0) is 0 by its own guard (arctan2 gives 0 or pi by the zeros\' signs)'
    d = got - np.arctan2(y.astype(np.float64), x.astype(np.float64))
    d = np.abs((d + np.pi) % (2 * np.pi) - np.pi)
    d = np.minimum(d, 2 * np.pi - d)
    w = int(d.argmax())
    r = row('atan2_fast', len(y), d[w], ATAN2_BOUND, 'rad', f'(y, x) = ({y[w]!r}, {x[w]!r})')
    assert d[w] <= ATAN2_BOUND, r
    return [r]


# two-term Cody-Waite reduction, |x| <= 100 (k <= 64): the first fma is exact (k * C1 has <= 29 bits and cancels against x down to a multiple of 2^-22
# below 1), the second rounds once (<= 2^-25 for |r| < 1), and C1 + fl(C2) misses pi/2 by < 1e-14 per quarter turn; sin and cos have slope <= 1
SINCOS_BOUND = 2 * U23 + 2.0 ** -25 + 64 * 1e-14


def check_sincos(be):
    rng = np.random.default_rng(9)
    k = np.arange(-127, 128)
    base = (k * (np.pi / 4)).astype(np.float32)   # every multiple of pi/4 up to 100: rintf's ties (odd k) and the quadrant switches
    X = [base]
    for step in (1, 2):
        up, dn = base.copy(), base.copy()
        for _ in range(step):
            up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
        X += [up, dn]
    X += [np.array([0.0, -0.0, 1e-30, -1e-30, 1e-10, 1e-4, -1e-4, 100.0, -100.0], np.float32), rng.uniform(-100, 100, 4096).astype(np.float32),
          rng.uniform(-np.pi, np.pi, 2048).astype(np.float32)]
    x = np.concatenate(X).astype(np.float32)
    x = x[np.abs(x) <= 100.0]
    o = Out(x.shape, np.float32)
    s, c = be.run('sincos', x, len(x), o, o)
    x64 = x.astype(np.float64)
    es, ec = np.abs(s - np.sin(x64)), np.abs(c - np.cos(x64))
    ws, wc = int(es.argmax()), int(ec.argmax())
    rows = [row('sincos_small sin', len(x), es[ws], SINCOS_BOUND, 'abs', f'x = {x[ws]!r}'), row('sincos_small cos', len(x), ec[wc], SINCOS_BOUND, 'abs', f'x = {x[wc]!r}')]
    assert es[ws] <= SINCOS_BOUND and ec[wc] <= SINCOS_BOUND, rows
    return rows


def pow_ratio_bound(a, p, b, q):
    """relative: the exponent p log2 a - q log2 b carries an absolute error of about 2^-23 (|p log2 a| + |q log2 b|) (v_log_f32 to 1 ulp, two
    products, one difference) which exp2 turns into a relative one (x ln 2), plus v_exp_f32's own ulp and the final rounding"""
    return (np.abs(p * np.log2(a)) + np.abs(q * np.log2(b)) + 2) * U22


POWERS = (1.0, 2.0, 2.5, 3.0, 5.0)


def check_pow_ratio(be):
    rng = np.random.default_rng(10)
    A, P, B, Q = [], [], [], []
    for pw in POWERS:
        a = np.concatenate([rng.uniform(1e-3, 1, 400), 10.0 ** rng.uniform(-3, 0, 200), [1.0, 1e-3, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))]])
        b = np.concatenate([rng.uniform(1e-4, 0.9999, len(a) - 3), [1e-4, 0.9999, 0.5]])
        A.append(a); B.append(b); P.append(np.full(len(a), pw)); Q.append(np.full(len(a), pw - 1))
    a, p, b, q = (np.concatenate(v).astype(np.float32) for v in (A, P, B, Q))
    got = be.run('pow_ratio', a, p, b, q, len(a), Out(a.shape, np.float32)).astype(np.float64)
    a64, p64, b64, q64 = (v.astype(np.float64) for v in (a, p, b, q))
    ref = a64 ** p64 / b64 ** q64
    err, bnd = np.abs(got - ref) / ref, pow_ratio_bound(a64, p64, b64, q64)
    w = _worst(err, bnd)
    r = row('fast_pow_ratio', len(a), err[w], bnd[w], 'rel', f'a = {a[w]!r} p = {p[w]} b = {b[w]!r} q = {q[w]}')
    assert (err <= bnd).all(), r
    return [r]


def getimpedance64(solimp, pos, margin):
    """mj_makeImpedance's getimpedance in float64 on the float32 inputs (the clamps are csrc/gq_step_kernel.h impedance()'s, which are MuJoCo's)"""
    s = np.asarray(solimp, np.float64)
    f = lambda v: float(np.float32(v))
    dmin, dmax = min(max(s[0], f(0.0001)), f(0.9999)), min(max(s[1], f(0.0001)), f(0.9999))
    width, mid, power = max(f(1e-15), s[2]), min(max(s[3], f(0.0001)), f(0.9999)), max(1.0, s[4])
    if dmin == dmax or width <= f(1e-15):
        return 0.5 * (dmin + dmax), 0.0, power, mid
    x = abs(float(np.float32(pos) - np.float32(margin))) / width   # pos - margin is one fp32 subtraction of the caller's values on both sides
    if x >= 1:
        return dmax, 1.0, power, mid
    if x <= 0:
        return dmin, 0.0, power, mid
    if power == 1:
        y = x
    elif x <= mid:
        y = x ** power / mid ** (power - 1)
    else:
        y = 1 - (1 - x) ** power / (1 - mid) ** (power - 1)
    return dmin + y * (dmax - dmin), x, power, mid


def check_impedance(be):
    """impedance() against getimpedance64.  The bound is absolute: x = |pos - margin| / width comes from fdiv (<= 2 ulp, + the rounding of the
    difference: <= 2^-22 relative), which moves y by at most power * 2^-22 (|dy/dx| <= power on either side of mid, the function is continuous
    at mid, 0 and 1, so a branch taken the other way at a border changes nothing); fast_pow_ratio adds its relative bound (y <= 1); the last
    multiply-add rounds twice."""
    rng = np.random.default_rng(13)
    S, POS, MAR = [], [], []
    for pw in POWERS:
        for mid in (0.5, 0.1, 0.9):
            for width in (2.0 ** -10, 0.05, 1e-15, 0.0):   # a power of two: x is exactly the value asked for; 1e-15 and below: the floor
                for (dmin, dmax) in ((0.9, 0.95), (0.5, 0.5), (0.2, 0.9999), (0.0, 1.0)):
                    m32 = np.float32(mid)
                    xs = [0.0, 1e-3, 1.0, 1.5, float(m32), float(np.nextafter(m32, np.float32(0))), float(np.nextafter(m32, np.float32(1)))] + list(rng.random(6))
                    for xx in xs:
                        S.append([dmin, dmax, width, mid, pw]); MAR.append(0.0); POS.append(-xx * max(width, 1e-15))
    S, POS, MAR = np.asarray(S, np.float32), np.asarray(POS, np.float32), np.asarray(MAR, np.float32)
    got = be.run('impedance', S, POS, MAR, len(S), Out(POS.shape, np.float32)).astype(np.float64)
    ref, bnd = np.zeros(len(S)), np.zeros(len(S))
    for i in range(len(S)):
        ref[i], x, pw, mid = getimpedance64(S[i], POS[i], MAR[i])
        a, b = (x, mid) if x <= mid else (1 - x, 1 - mid)
        epow = pow_ratio_bound(max(a, 1e-30), pw, b, pw - 1) if 0 < x < 1 else 0.0
        span = abs(float(min(max(np.float64(S[i, 1]), 1e-4), 0.9999)) - float(min(max(np.float64(S[i, 0]), 1e-4), 0.9999)))
        bnd[i] = span * (pw * U22 + epow) + 2 * U24
    err = np.abs(got - ref)
    w = _worst(err, bnd)
    r = row('impedance', len(S), err[w], bnd[w], 'abs', f'solimp = {S[w].tolist()} pos - margin = {float(POS[w] - MAR[w])!r}')
    assert (err <= bnd).all(), r
    return [r]


def check_qnormalize(be):
    """|norm - 1| <= 2 ulp of 1.0 (four squares and three sums: 2^-23 on n2, halved by the root; v_rsq_f32 1 ulp; the product half an ulp), each
    component within the same of q / |q|; the identity below |q|^2 = 1e-30; scales 1e-12 .. 1e12"""
    rng = np.random.default_rng(14)
    q = rng.normal(0, 1, (2048, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q *= 10.0 ** rng.choice([-12, -9, -6, -3, -1, 0, 0, 0, 1, 3, 6, 9, 12], 2048)[:, None] * rng.uniform(0.5, 2.0, 2048)[:, None]
    q[::64, 1:] = 0.0   # a pure scalar part
    small = rng.normal(0, 1, (64, 4)); small *= 1e-16 / np.linalg.norm(small, axis=1, keepdims=True)   # |q|^2 = 1e-32: the identity
    small[0] = 0.0
    q = np.concatenate([q, small]).astype(np.float32)
    got = be.run('qnormalize', q, len(q), Out(q.shape, np.float32)).astype(np.float64)
    q64 = q.astype(np.float64)
    n = np.linalg.norm(q64, axis=1)
    ident = n * n < 1e-31
    assert ident.sum() == 64 and (n[~ident] ** 2 > 1e-29).all()   # nothing sits at the threshold
    assert (got[ident] == [1, 0, 0, 0]).all(), 'qnormalize: identity below 1e-30'
    en = np.abs(np.linalg.norm(got[~ident], axis=1) - 1)
    ecmp = np.abs(got[~ident] - q64[~ident] / n[~ident, None]).max(1)
    wn, wc = int(en.argmax()), int(ecmp.argmax())
    rows = [row('qnormalize norm', (~ident).sum(), en[wn] / U23, 2.0, 'ulp of 1', f'q = {q[~ident][wn].tolist()}'),
            row('qnormalize components', (~ident).sum(), ecmp[wc] / U23, 2.0, 'ulp of 1', f'q = {q[~ident][wc].tolist()}')]
    assert en[wn] <= 2 * U23 and ecmp[wc] <= 2 * U23, rows
    return rows


SMALLEST_U1 = (46762216, 7, 3, 0x1a70, 1234, 0)   # found by search: word 0 of this block is < 256, so u1 = 2^-25, the smallest there is


def check_philox(be):
    """philox4x32 bit for bit against tests/philox_ref.py on 4096 counters with the env id, step and key words at 0, 1, 2^31 and 2^32 - 1;
    philox_normal against Box-Muller in float64 on the same words: |error| <= R (1e-6 + 4 * 2^-24), R = sqrt(-2 ln u1) - fast_cos_turns' bound
    times R, plus logf, sqrtf and the two products at about an ulp each"""
    from philox_ref import philox4x32
    rng = np.random.default_rng(15)
    edge = [0, 1, 1 << 31, (1 << 32) - 1]
    ck = rng.integers(0, 1 << 32, (4096, 6), dtype=np.uint64)
    k = 0
    for env in edge:          # counter word 2 = env id, word 1 = step, key words
        for step in edge:
            for k0 in edge:
                for k1 in edge:
                    ck[k, 1], ck[k, 2], ck[k, 4], ck[k, 5] = step, env, k0, k1; k += 1
    ck[:, 0] %= 64            # word 0 is a lane / draw index in the kernels
    ck[k] = SMALLEST_U1
    ck = ck.astype(np.uint32)
    words, z = be.run('philox', ck, len(ck), Out((len(ck), 4), np.uint32), Out((len(ck),), np.float32))
    ref = np.array([philox4x32(c[:4], c[4:]) for c in ck.tolist()], dtype=np.uint32)
    bad = np.nonzero((words != ref).any(1))[0]
    assert len(bad) == 0, ('philox4x32', ck[bad[0]], words[bad[0]], ref[bad[0]])
    assert ref[k, 0] >> 8 == 0, 'the smallest u1 is not in the table'
    u1 = ((ref[:, 0] >> 8).astype(np.float32) + np.float32(0.5)) * np.float32(1 / 16777216.0)
    u2 = (ref[:, 1] >> 8).astype(np.float32) * np.float32(1 / 16777216.0)
    R = np.sqrt(-2 * np.log(u1.astype(np.float64)))
    zr = R * np.cos(2 * np.pi * u2.astype(np.float64))
    err, bnd = np.abs(z - zr), R * (1e-6 + 4 * U24)
    w = _worst(err, bnd)
    rows = [row('philox4x32', len(ck), 0, 0, 'blocks off'), row('philox_normal', len(ck), err[w], bnd[w], 'abs', f'u1 = {u1[w]!r} u2 = {u2[w]!r}'),
            row('philox_normal (smallest u1)', 1, err[k], bnd[k], 'abs', f'u1 = {u1[k]!r} u2 = {u2[k]!r}')]
    assert (err <= bnd).all(), rows
    return rows


CHECKS = dict(wave_reduce=check_wave_reduce, wave_scan=check_wave_scan, lane_moves=check_lane_moves, ballot_bits=check_ballot_bits,
              unary=check_unary, fdiv=check_fdiv, med3=check_med3, atan2=check_atan2, sincos=check_sincos, pow_ratio=check_pow_ratio,
              impedance=check_impedance, qnormalize=check_qnormalize, philox=check_philox)


# ----------------------------------------------------------------------------------------------------------------- C. tree factor and solve
ROBOTS = ('mini_cheetah', 'aliengo', 'go1', 'go2', 'b2', 'hyqreal1', 'hyqreal2', 'spot')


def pack_tree(M):
    """dense 18 x 18 -> the kernel's tree-sparse storage (csrc/gq_step_kernel.h WaveMem::Mc, Mb)"""
    Mc, Mb = np.zeros((12, 9), np.float32), np.asarray(M[:6, :6], np.float32).copy()
    for j in range(12):
        d, leg, link = 6 + j, j // 3, j % 3
        Mc[j, :6] = M[d, :6]
        for a in range(link + 1):
            Mc[j, 6 + a] = M[d, 6 + 3 * leg + a]
    return Mc, Mb


def unpack_tree(Mc, Mb):
    M = np.zeros((18, 18))
    M[:6, :6] = np.tril(Mb.astype(np.float64)) + np.tril(Mb.astype(np.float64), -1).T
    for j in range(12):
        d, leg, link = 6 + j, j // 3, j % 3
        M[d, :6] = M[:6, d] = Mc[j, :6]
        for a in range(link + 1):
            M[d, 6 + 3 * leg + a] = M[6 + 3 * leg + a, d] = Mc[j, 6 + a]
    return M


@functools.lru_cache(None)
def tree_cases():
    """the oracle's mass matrix of all eight robots at 8 random poses each, in the kernel's storage (fp32), the model's damping, h = 0.002 and
    64 right-hand sides per system: the 18 unit vectors and 46 random ones; references by numpy.linalg.solve in float64 on the same fp32 data"""
    from helpers import marshalled, random_states
    from oracle.oracle import Oracle
    rng = np.random.default_rng(16)
    h = np.float32(0.002)
    MC, MB, D, RHS, X0, X1, COND, NAME = [], [], [], [], [], [], [], []
    for robot in ROBOTS:
        mm = marshalled(robot)
        o = Oracle(mm)
        damp = np.asarray(mm.md.dof_damping, np.float32)
        qpos, qvel = random_states(mm.md, 8, rng)
        for e in range(8):
            o.set_state(qpos[e], qvel[e], np.zeros(18), np.zeros(18), 0.0, -1.0)
            o.forward(np.zeros(12), stage=1)
            Mc, Mb = pack_tree(o.M)
            M = unpack_tree(Mc, Mb)
            rhs = np.concatenate([np.eye(18), rng.normal(0, 1, (46, 18))]).astype(np.float32)
            Md = M + float(h) * np.diag(damp.astype(np.float64))
            MC.append(Mc); MB.append(Mb); D.append(damp); RHS.append(rhs); NAME.append(f'{robot} pose {e}')
            X0.append(np.linalg.solve(M, rhs.astype(np.float64).T).T); X1.append(np.linalg.solve(Md, rhs.astype(np.float64).T).T)
            COND.append((np.linalg.cond(M), np.linalg.cond(Md)))
    return dict(Mc=np.stack(MC), Mb=np.stack(MB), damping=np.stack(D), h=float(h), rhs=np.stack(RHS), x0=np.stack(X0), x1=np.stack(X1),
                cond=np.asarray(COND), name=NAME)


def check_tree(be):
    """factor_tree_both + solve_tree: |x - x64|_inf / |x64|_inf <= 32 cond_2 2^-24 for every system and right-hand side"""
    T = tree_cases()
    n = len(T['Mc'])
    o = Out(T['rhs'].shape, np.float32)
    x0, x1 = be.run('tree', T['Mc'], T['Mb'], T['damping'], T['h'], T['rhs'], n, o, o)
    rows, ok = [], True
    for name, x, ref, cond in (('factor/solve_tree M', x0, T['x0'], T['cond'][:, 0]), ('factor/solve_tree M + h D', x1, T['x1'], T['cond'][:, 1])):
        err = np.abs(x - ref).max(2) / np.abs(ref).max(2)          # [system][rhs]
        bnd = 32 * cond * U24
        ratio = err / bnd[:, None]
        s, r = np.unravel_index(int(ratio.argmax()), ratio.shape)
        rows.append(row(name, ratio.size, err[s, r], bnd[s], 'rel inf-norm', f'{T["name"][s]} rhs {r} (cond {cond[s]:.3g}, measured / bound {ratio[s, r]:.3g})'))
        ok = ok and bool((ratio <= 1).all())
    assert ok, rows
    return rows
