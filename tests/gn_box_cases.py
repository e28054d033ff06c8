"""What the CPU and the GPU tests of the box-constrained Gauss-Newton step share (no test of its own): the messages, the boxes of every
kind, the KKT certificate and the brute-force enumeration of active sets.

The step (mpc4rl_amd.qlearning.qlearning_gn_box_step, mpcrl_qlearning_gn_apply_box):
    delta = argmin 1/2 d' H d - lr bb' d,  l <= d <= u,   H = Gb + damping diag(Gb_aa > 0 ? Gb_aa : 1e-12 d_max),  Gb = G / n, bb = b / n.

The certificate (eps = 2^-53), on r = H delta - lr bb recomputed here in float64 from the message:
    tol_a = 4 (3 K + 1) eps (sum_c sqrt(H_aa H_cc) |delta_c| + lr |bb_a|)
the backward error of a Cholesky solve of K unknowns (|dH| <= (3 K + 1) eps |L| |L'| to first order, |L| |L'|_ac <= sqrt(H_aa H_cc) by
Cauchy-Schwarz on the rows of L), with a factor 4 for the sums that form the right-hand side and r itself.
    active 0:  l_a <= delta_a <= u_a and |r_a| <= tol_a;    active 1:  delta_a == l_a and r_a >= -tol_a;    active 2:  delta_a == u_a and r_a <= tol_a.
The minimiser of a strictly convex QP is unique, so this does not depend on the algorithm."""
import itertools

import numpy as np
import torch

EPS = 2.0 ** -53


def message(G, b, count):
    K = G.shape[0]
    return torch.as_tensor(np.concatenate([G[np.triu_indices(K)], b, [0.0], [float(count)]]))


def h_of(msg, K, damping):
    """(H, bb) of a message in numpy float64, from its upper triangle as the kernel reads it."""
    m = np.asarray(msg, dtype=np.float64)
    KK = K * (K + 1) // 2
    n = max(1.0, m[KK + K + 1])
    Gb = np.zeros((K, K))
    Gb[np.triu_indices(K)] = m[:KK] / n
    Gb = Gb + np.triu(Gb, 1).T
    d = np.diag(Gb)
    return Gb + damping * np.diag(np.where(d > 0, d, 1e-12 * d.max())), m[KK: KK + K] / n


def box_of(lo, hi, scale, radius, theta):
    """l, u as the step defines them (numpy float64; radius * scale is one rounding)."""
    lo, hi, scale, theta = (np.asarray(t, dtype=np.float64) for t in (lo, hi, scale, theta))
    t = radius * scale
    return np.maximum(lo - theta, -t), np.minimum(hi - theta, t)


def certificate(msg, K, lr, damping, l, u, delta, active, what=""):
    """Asserts the KKT conditions of the module's docstring; returns the largest |r_a| / tol_a that was asked to be <= 1."""
    H, bb = h_of(msg, K, damping)
    delta, active = np.asarray(delta, dtype=np.float64), np.asarray(active)
    assert np.isfinite(delta).all(), what
    r = H @ delta - lr * bb
    root = np.sqrt(np.diag(H))
    tol = 4 * (3 * K + 1) * EPS * (root * (root @ np.abs(delta)) + lr * np.abs(bb))
    assert set(np.unique(active).tolist()) <= {0, 1, 2}, what
    f, a1, a2 = active == 0, active == 1, active == 2
    assert (delta[f] >= l[f]).all() and (delta[f] <= u[f]).all(), what
    assert (delta[a1] == l[a1]).all() and (delta[a2] == u[a2]).all(), what
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(f, np.abs(r), np.where(a1, -r, r)) / tol
    ratio = np.where(np.isnan(ratio), 0.0, ratio)                   # 0 / 0: r_a = 0 = tol_a
    worst = float(ratio.max())
    print(f"{what}: free {int(f.sum())} at l {int(a1.sum())} at u {int(a2.sum())}, largest wrong-signed r / tol {worst:.3e}")
    assert (np.abs(r[f]) <= tol[f]).all(), what
    assert (r[a1] >= -tol[a1]).all() and (r[a2] <= tol[a2]).all(), what
    return worst


def agree(delta, active, ref_delta, ref_active, msg, K, damping, what=""):
    """Two solutions of one problem: equal active sets, the same bits on the active entries, and on the free block
    ||d - d_ref||_2 <= 8 K (K + 1) eps cond_2(H_FF) ||d_ref||_2 (backward stability of Cholesky, on both sides)."""
    delta, ref_delta = np.asarray(delta, dtype=np.float64), np.asarray(ref_delta, dtype=np.float64)
    active, ref_active = np.asarray(active), np.asarray(ref_active)
    assert np.array_equal(active, ref_active), (what, active, ref_active)
    on = active != 0
    assert np.array_equal(delta[on], ref_delta[on]), what
    if (~on).any():
        H, _ = h_of(msg, K, damping)
        F = np.nonzero(~on)[0]
        err = np.linalg.norm(delta[F] - ref_delta[F])
        bound = 8 * K * (K + 1) * EPS * np.linalg.cond(H[np.ix_(F, F)]) * np.linalg.norm(ref_delta[F])
        print(f"{what}: free block {F.size}, difference {err:.3e}, bound {bound:.3e}")
        assert err <= bound, what


def brute_force(H, g, l, u):
    """All 3^K active sets: every entry free, at l or at u.  Solves each candidate's free block with numpy and keeps the feasible ones
    whose multipliers have the right signs; returns the one with the lowest objective as (delta, active) (they coincide unless the
    problem is degenerate)."""
    K = H.shape[0]
    best = None
    for act in itertools.product((0, 1, 2), repeat=K):
        act = np.array(act)
        if not (np.isfinite(l[act == 1]).all() and np.isfinite(u[act == 2]).all()):
            continue
        x = np.where(act == 1, l, np.where(act == 2, u, 0.0))
        F, B = np.nonzero(act == 0)[0], np.nonzero(act != 0)[0]
        if F.size:
            x[F] = np.linalg.solve(H[np.ix_(F, F)], g[F] - H[np.ix_(F, B)] @ x[B])
            if (x[F] < l[F]).any() or (x[F] > u[F]).any():
                continue
        r = H @ x - g
        if (r[act == 1] < 0).any() or (r[act == 2] > 0).any():
            continue
        obj = 0.5 * x @ H @ x - g @ x
        if best is None or obj < best[0]:
            best = (obj, x, act)
    assert best is not None
    return best[1], best[2]


def correlated_problem(K, seed):
    """H = A' A, A [K + 1, K] standard normal, a standard normal bb, count 1, and a box of +-0.3: correlated enough that the optimal active
    set is often not the set of entries the unconstrained step violates."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(K + 1, K))
    return A.T @ A, rng.normal(size=K), np.full(K, -0.3), np.full(K, 0.3)


def make_cases(G, b, count, K, lr, damping, seed):
    """The boxes of every kind for one message: a list of dicts with msg, lo, hi, scale, theta [K] (at the learned entries), radius, and
    `expect`: "free" (no bound active), "all" (every bound active) or None.  Built from the unconstrained step d0 of the torch statement."""
    from mpc4rl_amd import qlearning_gn_box_step
    rng = np.random.default_rng(seed)
    msg = message(G, b, count)
    theta = rng.normal(size=K)
    inf, one = np.full(K, np.inf), np.ones(K)
    d0, act0, info0 = qlearning_gn_box_step(msg, K, lr, damping, -inf, inf, one, np.inf, theta)
    assert info0 == 0 and int(act0.sum()) == 0
    d0 = d0.numpy()
    mag = np.abs(d0) + 1e-3 * np.abs(d0).max()
    scale = mag * rng.uniform(0.5, 2.0, K)
    cases = [dict(name="unbounded", lo=-inf, hi=inf, scale=one, radius=np.inf, expect="free"),
             dict(name="loose", lo=theta - 3 * mag, hi=theta + 3 * mag, scale=scale, radius=7.0, expect="free"),
             dict(name="tiny radius", lo=theta - 3 * mag, hi=theta + 3 * mag, scale=scale, radius=1e-8, expect="all")]
    c_lo, c_hi = rng.uniform(0.2, 2.0, K), rng.uniform(0.2, 2.0, K)
    mix = dict(name="mix", lo=theta - c_lo * mag, hi=theta + c_hi * mag, scale=one, radius=np.inf, expect=None)
    cases.append(mix)
    t = int(rng.integers(K))
    fixed = dict(mix, name="l = u", lo=mix["lo"].copy(), hi=mix["hi"].copy(), scale=scale, radius=3.0)
    fixed["lo"][t] = fixed["hi"][t] = theta[t] + 0.5 * d0[t]
    cases.append(fixed)
    out = dict(mix, name="theta outside", lo=mix["lo"].copy(), hi=mix["hi"].copy())
    out["lo"][::2] = theta[::2] + 0.1 * mag[::2]                    # theta below lo: l > 0
    out["hi"][::2] = theta[::2] + 2.0 * mag[::2]
    out["hi"][1::3] = theta[1::3] - 0.2 * mag[1::3]                 # theta above hi: u < 0
    out["lo"][1::3] = -np.inf
    cases.append(out)
    # the unconstrained solution exactly on a bound, in any arithmetic: an entry no term is sensitive to (a zero row, column and b_a, as
    # the chain's L has) steps by exactly 0, and its hi is theta itself.  K = 1: b = 0.
    Gz, bz = G.copy(), b.copy()
    if K == 1:
        bz[:] = 0.0
    else:
        Gz[t, :], Gz[:, t], bz[t] = 0.0, 0.0, 0.0
    tie = dict(name="on a bound", msg=message(Gz, bz, count), lo=theta - 3 * mag, hi=theta + 3 * mag, scale=one, radius=np.inf, expect=None)
    tie["hi"] = tie["hi"].copy()
    tie["hi"][t] = theta[t]
    cases.append(tie)
    for c in cases:
        c.setdefault("msg", msg)
        c["theta"] = theta
    return cases
