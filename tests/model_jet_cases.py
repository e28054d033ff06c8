"""Reference, yardstick and evaluation points for the dynamics jets (tests/test_model_jets_cpu.py, tests/test_gpu_model_jets.py).  CPU only.

The reference is a second-order forward-mode scalar over mpmath numbers at 50 digits (MpJet: value, gradient, full Hessian over all of
z = (u, x, theta)) run through plain RK4 of the model ODEs, which are written out here from their equations:

  cartpole (x, xdot, th, thdot; theta = (M, m, l); g = 9.8):
      temp  = (u + m thdot^2 sin th) / (m + M)
      thdd  = (g sin th - cos th temp) / (l (4/3 - m cos^2 th / (m + M)))
      xdd   = temp - m thdd cos th / (m + M)
  linear system (theta = (A column-major, B, b)):   x+ = A x + B u + b      (a discrete map: no integrator)

Every block the device evaluations yield is a slice or a contraction of that one Hessian (blocks()).  The yardstick is the same
construction over IEEE doubles (NpJet: numpy float64, / and np.sin / np.cos): its error against the reference is what an honest
fp64 evaluation of these formulas loses at a point, and the device is held to a small multiple of it.

Reference values are handed out as double-double pairs (hi, lo): dev - hi is exact for a dev near hi, so (dev - hi) - lo is the
device's error to ~1e-32 relative without any mpmath arithmetic per comparison."""
import functools
from types import SimpleNamespace

import numpy as np
from mpmath import mp, mpf

mp.dps = 50
N_POINTS = 67          # one full wavefront and a partial one
G = 9.8                # the double the kernels multiply with

DIMS = {"cartpole": SimpleNamespace(nx=4, nu=1, ntd=3, lin_coord=(0, 3, 4)),
        "linear": SimpleNamespace(nx=2, nu=1, ntd=8, lin_coord=(0, 1, 2))}


# ---- second-order forward mode ---------------------------------------------------------------------------------------------------
class MpJet:
    """value v, gradient g[n], Hessian h[n][n] (lower triangle stored, j <= i) of a scalar function of n variables, mpmath numbers"""
    __slots__ = ("v", "g", "h")

    def __init__(self, v, g, h):
        self.v, self.g, self.h = v, g, h

    @classmethod
    def const(cls, c, n):
        return cls(mpf(c), [mpf(0)] * n, [[mpf(0)] * (i + 1) for i in range(n)])

    @classmethod
    def var(cls, c, i, n):
        r = cls.const(c, n)
        r.g = list(r.g)
        r.g[i] = mpf(1)
        return r

    def _lift(self, o):
        return o if isinstance(o, MpJet) else MpJet.const(o, len(self.g))

    def _chain(self, f0, f1, f2):      # f(self) from f, f', f'' at self.v
        g, h = self.g, self.h
        return MpJet(f0, [f1 * a for a in g], [[f1 * h[i][j] + f2 * g[i] * g[j] for j in range(i + 1)] for i in range(len(g))])

    def __add__(self, o):
        if not isinstance(o, MpJet):
            return MpJet(self.v + o, self.g, self.h)
        return MpJet(self.v + o.v, [a + b for a, b in zip(self.g, o.g)], [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(self.h, o.h)])

    def __neg__(self):
        return MpJet(-self.v, [-a for a in self.g], [[-a for a in r] for r in self.h])

    def __sub__(self, o):
        if not isinstance(o, MpJet):
            return MpJet(self.v - o, self.g, self.h)
        return MpJet(self.v - o.v, [a - b for a, b in zip(self.g, o.g)], [[a - b for a, b in zip(ra, rb)] for ra, rb in zip(self.h, o.h)])

    def __mul__(self, o):
        if not isinstance(o, MpJet):
            return MpJet(self.v * o, [a * o for a in self.g], [[a * o for a in r] for r in self.h])
        a, b, ag, bg, ah, bh = self.v, o.v, self.g, o.g, self.h, o.h
        return MpJet(a * b, [x * b + a * y for x, y in zip(ag, bg)],
                     [[ah[i][j] * b + ag[i] * bg[j] + ag[j] * bg[i] + a * bh[i][j] for j in range(i + 1)] for i in range(len(ag))])

    def __truediv__(self, o):
        o = self._lift(o)
        r = 1 / o.v
        return self * o._chain(r, -r * r, 2 * r * r * r)

    __radd__, __rmul__ = __add__, __mul__

    def __rsub__(self, o):
        return self._lift(o) - self

    def __rtruediv__(self, o):
        return self._lift(o) / self

    def sincos(self):
        s, c = mp.sin(self.v), mp.cos(self.v)
        return self._chain(s, c, -s), self._chain(c, -s, -c)

    def hess(self, i, j):
        return self.h[i][j] if j <= i else self.h[j][i]


class NpJet:
    """the same scalar over IEEE doubles: v float64, g ndarray[n], h ndarray[n][n] (full, symmetric)"""
    __slots__ = ("v", "g", "h")

    def __init__(self, v, g, h):
        self.v, self.g, self.h = v, g, h

    @classmethod
    def const(cls, c, n):
        return cls(np.float64(c), np.zeros(n), np.zeros((n, n)))

    @classmethod
    def var(cls, c, i, n):
        r = cls.const(c, n)
        r.g[i] = 1.0
        return r

    def _lift(self, o):
        return o if isinstance(o, NpJet) else NpJet.const(o, len(self.g))

    def _chain(self, f0, f1, f2):
        return NpJet(f0, f1 * self.g, f1 * self.h + f2 * np.outer(self.g, self.g))

    def __add__(self, o):
        if not isinstance(o, NpJet):
            return NpJet(self.v + o, self.g, self.h)
        return NpJet(self.v + o.v, self.g + o.g, self.h + o.h)

    def __neg__(self):
        return NpJet(-self.v, -self.g, -self.h)

    def __sub__(self, o):
        o = self._lift(o)
        return NpJet(self.v - o.v, self.g - o.g, self.h - o.h)

    def __mul__(self, o):
        if not isinstance(o, NpJet):
            return NpJet(self.v * o, self.g * o, self.h * o)
        return NpJet(self.v * o.v, self.g * o.v + self.v * o.g, self.h * o.v + np.outer(self.g, o.g) + np.outer(o.g, self.g) + self.v * o.h)

    def __truediv__(self, o):
        o = self._lift(o)
        r = np.float64(1.0) / o.v
        return self * o._chain(r, -r * r, 2.0 * r * r * r)

    __radd__, __rmul__ = __add__, __mul__

    def __rsub__(self, o):
        return self._lift(o) - self

    def __rtruediv__(self, o):
        return self._lift(o) / self

    def sincos(self):
        s, c = np.sin(self.v), np.cos(self.v)
        return self._chain(s, c, -s), self._chain(c, -s, -c)

    def hess(self, i, j):
        return self.h[i, j]


# ---- the models, for any scalar with + - * / and sincos (MpJet, NpJet) or, with the two functions given, plain numbers --------------
def cartpole_ode(x, u, th, sincos, four_thirds):
    M, m, l = th
    s, c = sincos(x[2])
    total = m + M
    temp = (u[0] + m * x[3] * x[3] * s) / total
    thdd = (G * s - c * temp) / (l * (four_thirds - m * c * c / total))
    return [x[1], temp - m * thdd * c / total, x[3], thdd]


def linear_map(x, u, th):
    return [th[0] * x[0] + th[2] * x[1] + th[4] * u[0] + th[6], th[1] * x[0] + th[3] * x[1] + th[5] * u[0] + th[7]]


def rk4(ode, x, h, steps):
    """plain RK4: k1 .. k4 and x + h / 6 (k1 + 2 k2 + 2 k3 + k4), `steps` times"""
    for _ in range(steps):
        k1 = ode(x)
        k2 = ode([a + (h / 2) * k for a, k in zip(x, k1)])
        k3 = ode([a + (h / 2) * k for a, k in zip(x, k2)])
        k4 = ode([a + h * k for a, k in zip(x, k3)])
        x = [a + (h / 6) * (p + 2 * q + 2 * r + w) for a, p, q, r, w in zip(x, k1, k2, k3, k4)]
    return x


def disc_map(model, x, u, th, h, steps, sincos, four_thirds):
    """h and four_thirds (4 / 3) in the arithmetic of the scalars"""
    if model == "linear":
        return linear_map(x, u, th)
    return rk4(lambda xs: cartpole_ode(xs, u, th, sincos, four_thirds), x, h, steps)


def plain_map_mp(model, z, h, steps):
    """The map on plain mpmath numbers at the CURRENT working precision (mpmath.diff raises it): z = (u, x, theta) -> F[nx]"""
    d = DIMS[model]
    z = [mpf(a) for a in z]
    return disc_map(model, z[d.nu:d.nu + d.nx], z[:d.nu], z[d.nu + d.nx:], mpf(h), steps, lambda a: (mp.sin(a), mp.cos(a)), mpf(4) / 3)


def jet_map(kind, model, z, h, steps):
    """F[nx] as jets over all of z = (u, x, theta); kind = "mp" (reference) or "np" (yardstick)"""
    d = DIMS[model]
    J = MpJet if kind == "mp" else NpJet
    n = len(z)
    v = [J.var(z[i], i, n) for i in range(n)]
    hh, ft = (mpf(h), mpf(4) / 3) if kind == "mp" else (float(h), 4.0 / 3.0)
    return disc_map(model, v[d.nu:d.nu + d.nx], v[:d.nu], v[d.nu + d.nx:], hh, steps, lambda a: a.sincos(), ft)


# ---- evaluation points -----------------------------------------------------------------------------------------------------------
PI = float(np.pi)
HAND_ANGLES = [0.0, PI / 2, PI, 2 * PI, 7 * PI, -7 * PI, 25 * PI, -25 * PI]
HAND_ANGLES += [a + s * 1e-8 for a in HAND_ANGLES[:8] for s in (1.0, -1.0)]
HAND_RATES = [0.0, 15.0, -15.0]
HAND_CONTROLS = [0.0, 30.0, -30.0]
NOMINAL = (1.0, 0.1, 0.5)
HAND_THETAS = [NOMINAL, (1.5, 0.15, 0.75), (0.5, 0.05, 0.25), (1.0, 0.01, 0.5), (1.0, 0.1, 0.1)]
LINEAR_REFERENCE_THETA = (1.0, 0.0, 0.25, 1.0, 0.03125, 0.25, 0.0, 0.0)     # linear_system_ocp(): A column-major, B, b


def cartpole_points():
    """x [67][4], u [67][1], th [67][3]: the hand-picked angles (each with a hand-picked rate, control and parameter set, walked through
    at different strides so that they mix), ten angles in the reset range (0.9 .. 1.1) pi, and random points of a wound-up swing-up"""
    rng = np.random.default_rng(20240517)
    x, u, th = np.zeros((N_POINTS, 4)), np.zeros((N_POINTS, 1)), np.zeros((N_POINTS, 3))
    nh = len(HAND_ANGLES)
    for i, a in enumerate(HAND_ANGLES):
        x[i] = [0.3 * (i % 5) - 0.6, 0.7 * (i % 4) - 1.0, a, HAND_RATES[i % 3]]
        u[i, 0] = HAND_CONTROLS[(i // 3) % 3]
        th[i] = HAND_THETAS[i % 5]
        # Pole at rest, no force, angle within 1e-8 of a multiple of pi: an equilibrium to 1e-8, where dF/dtheta and the second
        # derivatives are O(1e-8) and come from the sine of a stage angle that was rounded at |angle| 2^-53 ~ 1e-15 -- any fp64
        # evaluation loses 1e-7 of them there.  The bar of the device tests is the yardstick's worst point, so one such point would
        # lower it to 1e-7 for every point; the angle keeps its place in the list with the force on.  (The origin below stays: there
        # these blocks are exact zeros.)
        if i > 0 and x[i, 3] == 0.0 and u[i, 0] == 0.0:
            u[i, 0] = HAND_CONTROLS[1 + i % 2]
    x[0] = 0.0      # the origin: angle, rates, control all exactly 0, nominal parameters
    u[0] = 0.0
    for i in range(nh, nh + 10):
        x[i] = [rng.uniform(-2.4, 2.4), rng.uniform(-10, 10), rng.uniform(0.9 * PI, 1.1 * PI), rng.uniform(-15, 15)]
        u[i, 0] = rng.uniform(-30, 30)
        th[i] = HAND_THETAS[i % 5]
    for i in range(nh + 10, N_POINTS):
        x[i] = [rng.uniform(-2.4, 2.4), rng.uniform(-10, 10), rng.uniform(-8 * PI, 8 * PI), rng.uniform(-15, 15)]
        u[i, 0] = rng.uniform(-30, 30)
        th[i] = np.array(NOMINAL) * rng.uniform(0.5, 1.5, 3)
    return x, u, th


def linear_points():
    """x [67][2], u [67][1], th [67][8]: the reference parameters and random ones of order 1; states and controls of order 1 and 1e3"""
    rng = np.random.default_rng(20240518)
    x, u, th = rng.standard_normal((N_POINTS, 2)), rng.standard_normal((N_POINTS, 1)), rng.standard_normal((N_POINTS, 8))
    th[:34] = LINEAR_REFERENCE_THETA
    x[1::2] *= 1e3
    u[1::2] *= 1e3
    return x, u, th


@functools.lru_cache(maxsize=None)
def case_set(name):
    """name -> model, h, rk_steps and the device inputs x, u, th, nu (aux of form 1), y (aux of form 3)"""
    model = "linear" if name == "linear" else "cartpole"
    d = DIMS[model]
    x, u, th = linear_points() if model == "linear" else cartpole_points()
    h, steps = {"cartpole": (0.025, 1), "cartpole_2step": (0.05, 2), "linear": (0.0, 1)}[name]
    rng = np.random.default_rng(7 + len(name))
    nu, y = rng.standard_normal((N_POINTS, d.nx)), rng.standard_normal((N_POINTS, d.nu + d.nx))
    for a in (x, u, th, nu, y):
        a.setflags(write=False)
    return SimpleNamespace(name=name, model=model, dims=d, h=h, rk_steps=steps, x=x, u=u, th=th, nu=nu, y=y, n=N_POINTS)


CASE_SETS = ("cartpole", "cartpole_2step", "linear")
BLOCKS = {0: ("F", "BA"), 1: ("F", "BA", "H", "hdd"), 2: ("F", "Fth"), 3: ("F", "e", "g", "m")}


def row_layout(model, which):
    """[(block, shape)] of one output row of mpcrl_debug_model_jets"""
    d = DIMS[model]
    nw, nh = d.nu + d.nx, len(d.lin_coord) * (len(d.lin_coord) + 1) // 2
    shapes = {"F": (d.nx,), "BA": (d.nx, nw), "H": (d.nx, nh), "hdd": (nh,), "Fth": (d.nx, d.ntd), "e": (d.nx,), "g": (d.nx, d.ntd),
              "m": (d.nx, d.ntd)}
    return [(b, shapes[b]) for b in BLOCKS[which]]


def split_row(model, which, rows):
    """rows [n][row] -> {block: [n][...]}"""
    out, o = {}, 0
    for b, shp in row_layout(model, which):
        sz = int(np.prod(shp))
        out[b] = rows[:, o:o + sz].reshape((rows.shape[0],) + shp)
        o += sz
    assert o == rows.shape[1]
    return out


def row_size(model, which):
    return sum(int(np.prod(shp)) for _, shp in row_layout(model, which))


def blocks(F, cs, i, kind):
    """Every block of every form at point i from the jets F[nx] over z = (u, x, theta): slices and contractions of the one Hessian.
    The contractions are carried out in the arithmetic of `kind`."""
    d = cs.dims
    nw, lc = d.nu + d.nx, d.lin_coord
    conv = mpf if kind == "mp" else np.float64
    y, nu = [conv(a) for a in cs.y[i]], [conv(a) for a in cs.nu[i]]
    H = [[f.hess(lc[a], lc[b]) for a in range(len(lc)) for b in range(a + 1)] for f in F]
    Fth = [[f.g[nw + t] for t in range(d.ntd)] for f in F]
    return {"F": [f.v for f in F],
            "BA": [[f.g[j] for j in range(nw)] for f in F],
            "H": H,
            "hdd": [sum((nu[m] * H[m][e] for m in range(d.nx)), conv(0)) for e in range(len(H[0]))],
            "Fth": Fth,
            "e": [sum((f.g[j] * y[j] for j in range(nw)), conv(0)) for f in F],
            "g": Fth,
            "m": [[sum((f.hess(nw + t, j) * y[j] for j in range(nw)), conv(0)) for t in range(d.ntd)] for f in F]}


def _z(cs, i):
    return [float(a) for a in np.concatenate([cs.u[i], cs.x[i], cs.th[i]])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """{block: (hi, lo)} float64 arrays [n][...] with hi + lo the 50-digit reference, and "jets": the per-point MpJet lists"""
    cs = case_set(name)
    per_point, jets = [], []
    for i in range(cs.n):
        F = jet_map("mp", cs.model, _z(cs, i), cs.h, cs.rk_steps)
        jets.append(F)
        per_point.append(blocks(F, cs, i, "mp"))
    out = {"jets": jets}
    for b in per_point[0]:
        obj = np.array([p[b] for p in per_point], dtype=object)
        hi = np.vectorize(float, otypes=[np.float64])(obj)
        lo = np.vectorize(lambda a, c: float(a - mpf(c)), otypes=[np.float64])(obj, hi)
        hi.setflags(write=False), lo.setflags(write=False)
        out[b] = (hi, lo)
    return out


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """{block: float64 [n][...]}: the same blocks from the float64 jets"""
    cs = case_set(name)
    per_point = [blocks(jet_map("np", cs.model, _z(cs, i), cs.h, cs.rk_steps), cs, i, "np") for i in range(cs.n)]
    out = {b: np.array([p[b] for p in per_point], dtype=np.float64) for b in per_point[0]}
    for a in out.values():
        a.setflags(write=False)
    return out


def block_errors(got, ref):
    """Per point: max |got - ref| / max |ref| over the block.  The denominator has the floor (largest |ref| of the block over all
    points) x 1e-300; a block that is zero at every point has to be reproduced exactly (error 0, or inf).
    Returns (err [n], absolute difference [n][...])."""
    hi, lo = ref
    n = hi.shape[0]
    diff = np.abs((np.asarray(got, dtype=np.float64) - hi) - lo).reshape(n, -1)
    scale = np.abs(hi).reshape(n, -1).max(axis=1)
    scale = np.maximum(scale, scale.max() * 1e-300)
    worst = diff.max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(scale > 0, worst / scale, np.where(worst == 0, 0.0, np.inf))
    return err, diff.reshape(hi.shape)


def rcp_inputs():
    """4096 doubles: random mantissas at exponents -20 .. 20 with both signs, and every power of two of that range with both signs"""
    rng = np.random.default_rng(4096)
    pw = np.ldexp(1.0, np.arange(-20, 21))
    pw = np.concatenate([pw, -pw])
    k = 4096 - pw.size
    r = np.ldexp(rng.uniform(1.0, 2.0, k), rng.integers(-20, 21, k)) * rng.choice([-1.0, 1.0], k)
    out = np.concatenate([r, pw])
    out.setflags(write=False)
    return out


def rcp_ulp_errors(x, got):
    """|got - 1 / x| in units of the last place of the correctly rounded 1 / x"""
    err = np.empty(len(x))
    for i, (a, b) in enumerate(zip(x, got)):
        exact = 1 / mpf(float(a))
        err[i] = float(abs(mpf(float(b)) - exact) / mpf(float(np.spacing(abs(float(exact))))))
    return err
