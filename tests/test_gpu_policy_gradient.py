"""GPU tests of the deterministic policy gradient with a compatible critic (csrc/cdpg_kernel.hpp, mpc4rl_amd/policy_gradient.py):
mpcrl_cdpg_record as an exact copy, mpcrl_cdpg_terms against its torch statement ``cdpg_terms`` on synthetic tables, mpcrl_cdpg_apply
against ``cdpg_step`` on the message the device holds, the argument checks, and the three learners end to end, eager and replayed from
graphs.

Bounds (derived, not measured), eps = 2^-53, M the number of terms:
  sums   |G_ac - G_ref,ac| <= (4 M + 2 nu + 2) eps sum_j (|J|'|d|)_ja (|J|'|d|)_jc: the 4 M eps sum_j |x_ja x_jc| of
         tests/test_gpu_qlearning_gn.py for a sum of M products in any order, on both sides, with |psi_ja| replaced by its own bound
         (|J|'|d|)_ja and 2 nu + 2 more roundings for the nu products and nu - 1 sums inside each of the two factors;
         b likewise with |delta_j| (|J|'|d|)_ja;  M_ac within 4 (M nu) eps sum_j sum_c' |J_jc'a J_jc'c| (M nu rows);  sum delta within
         4 M eps sum |delta_j|;  delta, valid and the count are exact.
  solve  ||w - w_ref||_2 <= 8 K (K + 1) eps cond_2(H) ||w_ref||_2 (backward stability of Cholesky, on both sides), H the damped matrix the
         message gives.  natural: step = -lr w, so ||step - ref||_2 <= 8 K (K + 1) eps cond_2(H) ||ref||_2.  Else step = -lr Mb w,
         Mb = M / n: step - ref = -lr Mb (w - w_ref) plus the product's own rounding, K eps lr ||Mb||_2 ||w||_2 at most, far below the
         first part's constant; so ||step - ref||_2 <= 8 K (K + 1) eps cond_2(H) lr ||Mb||_2 ||w_ref||_2.
The synthetic J spreads its columns over twelve orders of magnitude (10^-6 .. 10^6).  Every comparison prints its observed figure
beside the bound."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)
EPS = 2.0 ** -53
POISON = -7.0
E_ARG = -1


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _lib():
    from mpc4rl_amd import _lib
    return _lib.load()


def msg_len(K):
    return K * (K + 1) + K + 2


# ---------------------------------------------------------------------- record
@pytest.mark.parametrize("nu", [1, 3])
@pytest.mark.parametrize("E", [1, 5, 257])
def test_record_copies_the_rows_inside_the_table(E, nu):
    """row mixed over -1, 0, T - 1 and T: rows outside the table write nothing (the tables are poisoned first and compared bit for bit);
    the entry 9 of idx lies outside [0, n_p) and gives a zero column, as the negative one does."""
    lib = _lib()
    T, n_p, idx = 4, 7, [0, 5, 9, -2]
    K = len(idx)
    g = torch.Generator().manual_seed(E + nu)
    V, u0, du0 = torch.randn(E, generator=g, dtype=torch.float64), torch.randn(E, nu, generator=g, dtype=torch.float64), \
        torch.randn(E, nu, n_p, generator=g, dtype=torch.float64)
    du0[0, 0, 5] = float("nan")                                                   # copied as it is
    status = torch.randint(0, 5, (E,), generator=g, dtype=torch.int32)
    row = torch.tensor([(-1, 0, T - 1, T)[(e + 1) % 4] for e in range(E)], dtype=torch.int32)
    Vt, U0, Jt = torch.full((T, E), POISON, **F64), torch.full((T, E, nu), POISON, **F64), torch.full((T, E, nu, K), POISON, **F64)
    St = torch.full((T, E), 77, dtype=torch.int32, device=DEV)
    want = [t.cpu().clone() for t in (Vt, U0, St, Jt)]
    for e in range(E):
        r = int(row[e])
        if 0 <= r < T:
            want[0][r, e], want[1][r, e], want[2][r, e] = V[e], u0[e], status[e]
            for a, c in enumerate(idx):
                want[3][r, e, :, a] = du0[e, :, c] if 0 <= c < n_p else 0.0
    dev = [t.to(DEV) for t in (V, u0, du0, status, row, torch.tensor(idx, dtype=torch.int32))]
    assert lib.mpcrl_cdpg_record(*[_p(t) for t in dev], E, T, nu, n_p, K, _p(Vt), _p(U0), _p(St), _p(Jt), _stream()) == 0
    torch.cuda.synchronize()
    for got, w in zip((Vt, U0, St, Jt), want):
        got = got.cpu()
        if got.is_floating_point():                                                      # (the planted NaN is copied as it is)
            assert torch.equal(torch.isnan(got), torch.isnan(w))
            got, w = torch.nan_to_num(got), torch.nan_to_num(w)
        assert torch.equal(got, w)
    assert torch.equal(dev[4].cpu(), row)                                            # the rows are the collect launch's to advance


# ---------------------------------------------------------------------- terms
def make_tables(T, E, nu, K, seed, all_invalid=False):
    """Episode tables (CPU tensors) with every kind of term: live prefixes of every length, failed solves, NaN in v, u0 and J of every row
    that is dead or failed, the columns of J spread over twelve orders of magnitude.  The last environment is all valid."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, T + 1, E)
    L[rng.uniform(size=E) < 0.8] = T
    L[E - 1] = T
    if all_invalid:
        L[:] = 2
    live = (np.arange(T)[:, None] < L[None, :]).astype(np.uint8)
    cost = rng.uniform(0, 5, (T, E))
    v, u0 = rng.normal(size=(T, E)), rng.normal(size=(T, E, nu))
    act = u0 + 0.1 * rng.normal(size=(T, E, nu))
    J = rng.normal(size=(T, E, nu, K)) * 10.0 ** np.linspace(-6, 6, K)[rng.permutation(K)]
    status = np.where(rng.uniform(size=(T, E)) < 0.1, 2, 0).astype(np.int32)
    status[:, E - 1] = 0
    bad = (status != 0) | (live == 0)
    v[bad], u0[bad], J[bad] = np.nan, np.nan, np.nan
    return [torch.as_tensor(a) for a in (v, u0, J, status, act, cost, live)]


def run_terms(d, T, E, nu, K, gamma, launches=1):
    """mpcrl_cdpg_terms on the tables d (CPU tensors): (msg, delta, valid) of every launch, as CPU tensors."""
    lib = _lib()
    dev = [t.to(DEV).contiguous() for t in d]
    nb = lib.mpcrl_cdpg_workspace_bytes(T, E, K)
    assert nb > 0
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    out = []
    for _ in range(launches):
        msg = torch.full((msg_len(K),), POISON, **F64)
        delta = torch.full((max(T - 2, 0), E), POISON, **F64)
        valid = torch.full((max(T - 2, 0), E), 9, dtype=torch.uint8, device=DEV)
        assert lib.mpcrl_cdpg_terms(*[_p(t) for t in dev], T, E, nu, K, gamma, _p(ws), _p(delta), _p(valid), _p(msg), _stream()) == 0
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32)[0]) == 0                # the ticket is left zero
        out.append((msg.cpu(), delta.cpu(), valid.cpu()))
    return out


def sum_bounds(d, valid, delta, M):
    """The bounds of the module's text in the message's packing; 0 for the count."""
    v, u0, J, status, act, cost, live = d
    n_t, E = valid.shape
    nu, K = J.shape[-2], J.shape[-1]
    Ja = torch.nan_to_num(J[:n_t].reshape(n_t, E, nu, K)).abs()
    Ja = torch.where(valid[..., None, None], Ja, torch.zeros_like(Ja))
    da = (act[:n_t].reshape(n_t, E, nu) - u0[:n_t].reshape(n_t, E, nu)).abs()
    da = torch.where(valid[..., None], da, torch.zeros_like(da))
    pa = (Ja * da[..., None]).sum(2).reshape(-1, K)                                   # (|J|'|d|)_ja
    t = delta.abs().reshape(-1)
    Jr = Ja.reshape(-1, K)
    iu = torch.triu_indices(K, K)
    f = (4 * M + 2 * nu + 2) * EPS
    return torch.cat([f * (pa.t() @ pa)[iu[0], iu[1]], f * (pa.t() @ t), 4 * M * nu * EPS * (Jr.t() @ Jr)[iu[0], iu[1]],
                      4 * M * EPS * t.sum().reshape(1), torch.zeros(1, dtype=torch.float64)])


def check_message(got, d, gamma, M, what):
    from mpc4rl_amd import cdpg_terms
    msg, delta, valid = cdpg_terms(*d, gamma)
    bound = sum_bounds(d, valid, delta, M)
    assert torch.isfinite(got[0]).all(), what
    assert torch.equal(got[1], delta) and torch.equal(got[2].bool(), valid), what
    assert float(got[0][-1]) == float(valid.sum()), what
    diff = (got[0] - msg).abs()
    worst = float((diff / bound.clamp(min=1e-300))[:-1].max())
    print(f"{what}: count {int(valid.sum())} of {M}, largest difference / bound {worst:.3e}")
    assert bool((diff <= bound).all()), what
    return msg, delta, valid


@pytest.mark.parametrize("nu", [1, 3])
@pytest.mark.parametrize("K", [1, 15, 16, 17, 40, 64])
@pytest.mark.parametrize("T,E", [(3, 1), (3, 63), (3, 64), (3, 65), (3, 127), (3, 128), (3, 129), (12, 300)])
def test_terms_kernel_matches_torch_form(T, E, K, nu):
    """(T - 2) E terms: 1, around half a block (64 rows are staged at a time), around a block (128), and 3000: 24 blocks, all four slices
    of the final sum.  K at both sides of a column tile (16) and the cap.  Two launches give the same bits."""
    gamma, M = 0.97, (T - 2) * E
    d = make_tables(T, E, nu, K, 100 * T + 7 * E + K + nu)
    first, second = run_terms(d, T, E, nu, K, gamma, launches=2)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    _, _, valid = check_message(first, d, gamma, M, f"T {T} E {E} K {K} nu {nu}")
    assert int(valid.sum()) > 0 and (E < 60 or int(valid.sum()) < M)


def test_terms_of_an_all_invalid_table_and_of_two_rows():
    lib = _lib()
    T, E, nu, K = 5, 43, 3, 5
    d = make_tables(T, E, nu, K, 1, all_invalid=True)
    (msg, delta, valid), = run_terms(d, T, E, nu, K, 0.97)
    assert float(msg.abs().sum()) == 0.0 and float(delta.abs().sum()) == 0.0 and int(valid.sum()) == 0
    m0 = torch.full((msg_len(K),), POISON, **F64)                                    # T = 2: no term, an empty message
    assert lib.mpcrl_cdpg_terms(*[None] * 7, 2, E, nu, K, 0.9, None, None, None, _p(m0), _stream()) == 0
    torch.cuda.synchronize()
    assert float(m0.abs().sum()) == 0.0
    # such a message takes no step
    theta = torch.randn(9, generator=torch.Generator().manual_seed(0), dtype=torch.float64).to(DEV)
    theta0 = theta.clone()
    step, w = torch.full((9,), POISON, **F64), torch.full((K,), POISON, **F64)
    active, info = torch.full((K,), 9, dtype=torch.uint8, device=DEV), torch.full((1,), 7, dtype=torch.int32, device=DEV)
    idx_d = torch.arange(K, dtype=torch.int32, device=DEV)
    assert lib.mpcrl_cdpg_apply(_p(msg.to(DEV)), K, _p(idx_d), 9, 0.5, 1e-3, 0, None, None, None, float("inf"), _p(theta), _p(step), _p(w),
                                _p(active), _p(info), _stream()) == 0
    torch.cuda.synchronize()
    assert int(info) == -1 and torch.equal(theta, theta0) and float(step.abs().sum()) == 0.0 == float(w.abs().sum()) and int(active.sum()) == 0


# ---------------------------------------------------------------------- apply
def _idx(K):
    return [3 * a + 1 for a in range(K)]


def run_apply(msg, K, idx, n_theta, lr, damping, natural, lo=None, hi=None, scale=None, radius=float("inf"), theta0=None):
    """mpcrl_cdpg_apply on a message (CPU tensor): (step at idx, w, active, info, theta, theta0), and the checks every outcome shares."""
    lib = _lib()
    if theta0 is None:
        theta0 = torch.randn(n_theta, generator=torch.Generator().manual_seed(K), dtype=torch.float64)
    theta, step, w = theta0.to(DEV), torch.full((n_theta,), POISON, **F64), torch.full((K,), POISON, **F64)
    active, info = torch.full((K,), 9, dtype=torch.uint8, device=DEV), torch.full((1,), 7, dtype=torch.int32, device=DEV)
    idx_d = torch.tensor(idx, dtype=torch.int32, device=DEV)
    box = [None if t is None else t.to(DEV) for t in (lo, hi, scale)]
    assert lib.mpcrl_cdpg_apply(_p(msg.to(DEV)), K, _p(idx_d), n_theta, lr, damping, int(natural), *[_p(t) for t in box], radius, _p(theta), _p(step),
                                _p(w), _p(active), _p(info), _stream()) == 0
    torch.cuda.synchronize()
    step, theta, w, active, info = step.cpu(), theta.cpu(), w.cpu(), active.cpu(), int(info)
    off = torch.ones(n_theta, dtype=torch.bool)
    off[idx] = False
    assert float(step[off].abs().sum()) == 0.0 and torch.equal(theta[off], theta0[off])          # only theta[idx] may move
    if info != 0:
        assert torch.equal(theta, theta0) and float(step.abs().sum()) == 0.0 == float(w.abs().sum()) and int(active.sum()) == 0
    return step[idx], w, active, info, theta, theta0


def _spd_message(K, kappa, seed, n=37):
    rng = np.random.default_rng(seed)
    Qm = np.linalg.qr(rng.normal(size=(K, K)))[0]
    ev = np.logspace(0, -np.log10(kappa), K) if K > 1 else np.array([0.3])
    H = (Qm * ev) @ Qm.T
    H = 0.5 * (H + H.T)
    R = rng.normal(size=(2 * K + 3, K))
    Mm = R.T @ R / (2 * K + 3)
    iu = np.triu_indices(K)
    return torch.as_tensor(np.concatenate([(H * n)[iu], rng.normal(size=K) * n, (Mm * n)[iu], [0.0], [float(n)]])), n


def _h_and_mb(msg, K, damping):
    """The damped matrix and M / n of a message, in numpy (for the bounds)."""
    m = msg.numpy()
    KK = K * (K + 1) // 2
    n = max(1.0, m[-1])

    def unpack(tri):
        A = np.zeros((K, K))
        A[np.triu_indices(K)] = tri / n
        return A + np.triu(A, 1).T

    Gb, Mb = unpack(m[:KK]), unpack(m[KK + K: 2 * KK + K])
    dg = np.diag(Gb)
    return Gb + damping * np.diag(np.where(dg > 0, dg, 1e-12 * dg.max())), Mb


def step_bound(msg, K, lr, damping, natural, w_ref):
    Hd, Mb = _h_and_mb(msg, K, damping)
    return 8 * K * (K + 1) * EPS * np.linalg.cond(Hd) * lr * (1.0 if natural else np.linalg.norm(Mb, 2)) * float(w_ref.norm())


@pytest.mark.parametrize("natural", [True, False])
@pytest.mark.parametrize("kappa", [1e2, 1e6])
@pytest.mark.parametrize("K", [1, 12, 40, 64])
def test_apply_matches_torch_form(K, kappa, natural):
    from mpc4rl_amd import cdpg_step
    msg, n = _spd_message(K, kappa, K)
    idx, n_theta, lr = _idx(K), 3 * K + 5, 0.8
    for damping in (0.0, 1e-3):
        step, w, active, info, theta, theta0 = run_apply(msg, K, idx, n_theta, lr, damping, natural)
        ref, w_ref, _, info_t = cdpg_step(msg, K, lr, damping, natural)
        bound = step_bound(msg, K, lr, damping, natural, w_ref)
        e_s, e_w = float((step - ref).norm()), float((w - w_ref).norm())
        print(f"K {K} kappa {kappa:g} damping {damping:g} natural {natural}: step {e_s:.3e} (bound {bound:.3e}), w {e_w:.3e}")
        assert info == 0 == info_t and int(active.sum()) == 0 and float(ref.norm()) > 0.0
        assert e_s <= bound and e_w <= step_bound(msg, K, 1.0, damping, True, w_ref)
        assert torch.equal(theta[idx], theta0[idx] + step)


def test_apply_codes_leave_theta_untouched():
    from mpc4rl_amd import cdpg_step
    rng = np.random.default_rng(0)
    K, n = 5, 40
    psi = rng.normal(size=(n, K))
    psi[:, 3] = 0.0                                                 # an entry no term is sensitive to: G has a zero row and column
    G, b = psi.T @ psi, psi.T @ rng.normal(size=n)
    iu = np.triu_indices(K)
    mk = lambda Gm, count: torch.as_tensor(np.concatenate([Gm[iu], b, np.eye(K)[iu] * n, [0.0], [float(count)]]))
    idx, n_theta = _idx(K), 3 * K + 5
    step, w, active, info, *_ = run_apply(mk(G, n), K, idx, n_theta, 1.0, 0.0, True)
    assert info == 4 == cdpg_step(mk(G, n), K, 1.0, 0.0, True)[3]                             # pivot 3, 1-based
    step, w, active, info, *_ = run_apply(mk(G, n), K, idx, n_theta, 1.0, 1e-3, True)
    assert info == 0 and float(step[3]) == 0.0 and float(step.abs().sum()) > 0.0
    for bad in (mk(G, 0), mk(np.zeros((K, K)), n), mk(np.where(np.eye(K) > 0, np.nan, G), n)):
        assert run_apply(bad, K, idx, n_theta, 1.0, 1e-3, False)[3] == -1 == cdpg_step(bad, K, 1.0, 1e-3, False)[3]
    full = lambda v: torch.full((n_theta,), v, dtype=torch.float64)
    nan_lo = full(-9.0)
    nan_lo[idx[2]] = float("nan")
    for lo, hi in ((full(9.0), full(-9.0)), (nan_lo, full(9.0))):                              # an empty interval / a NaN bound
        assert run_apply(mk(G, n), K, idx, n_theta, 1.0, 1e-3, True, lo=lo, hi=hi)[3] == -2
    nan_sc = full(1.0)
    nan_sc[idx[0]] = float("nan")
    assert run_apply(mk(G, n), K, idx, n_theta, 1.0, 1e-3, True, scale=nan_sc, radius=1.0)[3] == -2


@pytest.mark.parametrize("natural", [True, False])
@pytest.mark.parametrize("K", [1, 12, 64])
def test_apply_clip_takes_the_bounds_bit_for_bit(K, natural):
    """Bounds and a trust region that cut about half of the entries: a clipped entry is its interval's end bit for bit (the statement's),
    the others are within the solve's bound, theta stays inside [lo, hi]; the three pointers may each be null."""
    from mpc4rl_amd import cdpg_step
    msg, n = _spd_message(K, 1e3, 50 + K)
    idx, n_theta, lr, damping = _idx(K), 3 * K + 5, 0.8, 1e-3
    free, w_ref, _, _ = cdpg_step(msg, K, lr, damping, natural)
    theta0 = torch.randn(n_theta, generator=torch.Generator().manual_seed(K), dtype=torch.float64)
    cut = torch.tensor([0.5 if a % 2 == 0 else 3.0 for a in range(K)], dtype=torch.float64) * free.abs()
    lo, hi, sc = torch.full((n_theta,), -np.inf, dtype=torch.float64), torch.full((n_theta,), np.inf, dtype=torch.float64), \
        torch.ones(n_theta, dtype=torch.float64)
    lo[idx], hi[idx], sc[idx] = theta0[idx] - cut, theta0[idx] + cut, cut
    bound = step_bound(msg, K, lr, damping, natural, w_ref)
    for kw in (dict(lo=lo, hi=hi), dict(scale=sc, radius=1.0), dict(lo=lo), dict(hi=hi, scale=sc, radius=4.0), dict(lo=lo, hi=hi, scale=sc, radius=0.5)):
        step, w, active, info, theta, _ = run_apply(msg, K, idx, n_theta, lr, damping, natural, theta0=theta0, **kw)
        at = lambda t: None if t is None else t[idx]
        ref, _, act_ref, info_t = cdpg_step(msg, K, lr, damping, natural, lo=at(kw.get("lo")), hi=at(kw.get("hi")), scale=at(kw.get("scale")),
                                            radius=kw.get("radius", float("inf")), theta_idx=theta0[idx])
        assert info == 0 == info_t and torch.equal(active, act_ref)
        if len(kw) != 1 and kw.get("radius") != 4.0:                                             # both sides are limited: every even entry is cut
            assert int((active != 0).sum()) == (K + 1) // 2
        on = active != 0
        assert torch.equal(step[on], ref[on])                                                   # the bound's own bits
        assert float((step[~on] - ref[~on]).norm()) <= bound
        if "lo" in kw:
            assert bool((theta >= lo).all())
        if "hi" in kw:
            assert bool((theta <= hi).all())
        if "scale" in kw:
            assert bool((step.abs() <= kw["radius"] * cut).all())


def test_argument_checks_return_e_arg_and_write_nothing():
    lib = _lib()
    T, E, nu, n_p, K = 4, 3, 3, 70, 3
    z = torch.full((4096,), POISON, **F64)
    zi = torch.zeros(64, dtype=torch.int32, device=DEV)
    rec = lambda E=E, T=T, nu=nu, K=K, **null: lib.mpcrl_cdpg_record(
        *[None if null.get(k) else _p(t) for k, t in (("V", z), ("u0", z), ("du0", z), ("status", zi), ("row", zi), ("idx", zi))], E, T, nu, n_p, K,
        *[None if null.get(k) else _p(t) for k, t in (("Vt", z), ("U0", z), ("St", zi), ("Jt", z))], _stream())
    ter = lambda E=E, T=T, nu=nu, K=K, **null: lib.mpcrl_cdpg_terms(
        *[None if null.get(k) else _p(t) for k, t in (("Vt", z), ("U0", z), ("Jt", z), ("St", zi), ("act", z), ("cost", z), ("live", zi))], T, E, nu, K,
        0.9, *[None if null.get(k) else _p(t) for k, t in (("ws", z), ("delta", z), ("valid", zi), ("msg", z))], _stream())
    app = lambda K=K, n_theta=n_p, lr=1.0, damping=0.0, radius=float("inf"), **null: lib.mpcrl_cdpg_apply(
        None if null.get("msg") else _p(z), K, None if null.get("idx") else _p(zi), n_theta, lr, damping, 0, None, None, None, radius,
        *[None if null.get(k) else _p(t) for k, t in (("theta", z), ("step", z), ("w", z), ("active", zi), ("info", zi))], _stream())
    for bad in (dict(K=0), dict(K=65), dict(K=-1), dict(nu=0), dict(nu=4), dict(T=1), dict(E=0)):
        assert rec(**bad) == E_ARG, bad
        assert ter(**bad) == E_ARG, bad
        if "K" in bad:
            assert app(**bad) == E_ARG and lib.mpcrl_cdpg_workspace_bytes(T, E, bad["K"]) == E_ARG, bad
    assert lib.mpcrl_cdpg_workspace_bytes(1, E, K) == E_ARG and lib.mpcrl_cdpg_workspace_bytes(T, 0, K) == E_ARG
    for name in ("V", "u0", "du0", "status", "row", "idx", "Vt", "U0", "St", "Jt"):
        assert rec(**{name: True}) == E_ARG, name
    for name in ("Vt", "U0", "Jt", "St", "act", "cost", "live", "ws", "delta", "msg"):
        assert ter(**{name: True}) == E_ARG, name
    for name in ("msg", "idx", "theta", "step", "w", "active", "info"):
        assert app(**{name: True}) == E_ARG, name
    for bad in (dict(n_theta=K - 1), dict(lr=float("nan")), dict(lr=float("inf")), dict(damping=-1.0), dict(damping=float("nan")), dict(radius=0.0),
                dict(radius=float("nan"))):
        assert app(**bad) == E_ARG, bad
    torch.cuda.synchronize()
    assert bool((z == POISON).all()) and int(zi.abs().sum()) == 0


# ---------------------------------------------------------------------- the learners
def _linear(graphs=False, **kw):
    from mpc4rl_amd import BatchedLinearSystemEnv, LinearPolicyGradient, linear_system_ocp
    pg = LinearPolicyGradient(linear_system_ocp(), BatchedLinearSystemEnv(8, device=DEV, seed=5), 6, noise_scale=0.1, seed=6, **kw)
    if graphs:
        pg.enable_graphs()
    return pg, None


def _chain(graphs=False, **kw):
    """The mismatch plant of tests/test_gpu_qlearning_gn.py: m x 1.1, D x 0.9."""
    from mpc4rl_amd import BatchedChainMassEnv, ChainPolicyGradient, chain_mass_ocp, chain_theta_bounds
    from mpc4rl_amd.problems import chain_param_layout
    ocp = chain_mass_ocp(3, N=10)
    off = chain_param_layout(3)[4]
    p = torch.tensor(ocp.p0)
    p[off["m"][0]: off["m"][1]] *= 1.1
    p[off["D"][0]: off["D"][1]] *= 0.9
    env = BatchedChainMassEnv(4, ocp, device=DEV, p=p, w_std=0.01, vel_std=1e-2, seed=1)
    pg = ChainPolicyGradient(ocp, env, 4, noise_scale=0.05, seed=2, theta_bounds=chain_theta_bounds(ocp), **kw)
    if graphs:
        pg.enable_graphs()
    return pg, None


def _cartpole(graphs=False, **kw):
    """The smallest shape of tests/test_gpu_qlearning_cartpole.py: E 8, T 40, truncation at 30 steps, two environments that start inside
    the goal box and end early."""
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, CartpolePolicyGradient, cartpole_ocp
    E = 8
    pg = CartpolePolicyGradient(cartpole_ocp(), BatchedCartPoleSwingUpEnv(E, device=DEV, seed=1, max_episode_steps=30), 40, noise_scale=0.1, seed=2,
                                **kw)
    if graphs:
        pg.enable_graphs()
    x0 = np.zeros((E, 4))
    x0[:, 2] = np.linspace(0.92, 1.08, E) * np.pi
    x0[0], x0[1] = [0.02, 0.0, 0.01, 0.0], [-0.03, 0.02, -0.01, 0.01]
    x0[2], x0[3] = [0.15, 0.0, 0.05, 0.0], [-0.1, 0.1, -0.04, 0.0]
    return pg, torch.as_tensor(x0, device=DEV)


def _check_episode(pg, st, theta0, K_want, all_valid):
    from mpc4rl_amd import cdpg_step
    T, E, NU = pg.T, pg.E, pg.NU
    idx = pg.learn_idx.cpu().tolist()
    assert len(idx) == pg.K == K_want and idx == torch.nonzero(pg.learn_mask.cpu()).reshape(-1).tolist()
    assert not hasattr(pg, "sample_mpc") and pg.last_sweep is None and len(pg.last) == T
    d = [torch.stack([r.V for r in pg.last]).cpu(), torch.stack([r.u0 for r in pg.last]).cpu(),
         torch.stack([r.dpi_dp for r in pg.last])[..., idx].cpu(), torch.stack([r.status for r in pg.last]).cpu(), pg.A.reshape(T, E, NU).cpu(),
         pg.C.cpu(), pg.live.cpu()]
    M = (T - 2) * E
    name = type(pg).__name__
    msg, delta, valid = check_message((pg.msg.cpu(), pg.delta.cpu(), pg.valid.cpu()), d, pg.gamma, M, name)
    count = int(valid.sum())
    assert count > 0 and float(pg.msg[-1]) == count
    if all_valid:
        assert count == M                                                             # no instance is left out
    assert abs(st.td_error_mean - float(delta.sum()) / count) <= 4 * M * EPS * float(delta.abs().sum()) / count + 1e-300
    # the step, on the message the device holds: only the factorisation and the product differ
    box = pg.box
    at = lambda t: t.cpu()[idx]
    ref, w_ref, act_ref, info = cdpg_step(pg.msg.cpu(), pg.K, pg.lr, pg.damping, pg.natural, lo=at(pg.theta_lo) if box else None,
                                          hi=at(pg.theta_hi) if box else None, scale=at(pg.theta_scale) if box else None,
                                          radius=pg.trust_radius, theta_idx=theta0.cpu()[idx])
    step = pg.step_out.cpu()
    bound = step_bound(pg.msg.cpu(), pg.K, pg.lr, pg.damping, pg.natural, w_ref)
    on = act_ref != 0
    err = float((step[idx][~on] - ref[~on]).norm())
    print(f"{name}: K {pg.K}, info {st.gn_info}, clipped {st.gn_active}, |step| {float(step.norm()):.3e}, step difference {err:.3e}, bound {bound:.3e}")
    assert st.gn_info == 0 == info and float(ref.norm()) > 0.0
    assert err <= bound and float((pg.w.cpu() - w_ref).norm()) <= step_bound(pg.msg.cpu(), pg.K, 1.0, pg.damping, True, w_ref)
    assert torch.equal(pg.gn_active.cpu(), act_ref) and torch.equal(step[idx][on], ref[on]) and st.gn_active == int(on.sum())
    off = torch.ones(pg.n_p, dtype=torch.bool)
    off[idx] = False
    assert float(step[off].abs().sum()) == 0.0 and torch.equal(st.step, pg.step_out)
    assert torch.equal(pg.theta, theta0 + pg.step_out)                                # (no bound on theta itself is met in one episode)
    assert torch.equal(pg.rollout_mpc.get_theta(), pg.theta)


@pytest.mark.parametrize("make,K,all_valid,kw", [(_linear, 12, True, dict(lr=0.05)),
                                                 (_chain, 20, True, dict(lr=0.5, natural=True, trust_radius=0.02)),
                                                 (_cartpole, 3, False, dict(lr=0.05, trust_radius=0.05))], ids=["linear", "chain", "cartpole"])
def test_policy_gradient_episode_eager_and_from_graphs(make, K, all_valid, kw):
    """One episode: the message against cdpg_terms on the learner's own roll-out solves and tables, the applied step against cdpg_step;
    the same episode replayed from graphs, from the same seeds, is the same bits."""
    runs = []
    for graphs in (False, True):
        pg, x0 = make(graphs=graphs, **kw)
        theta0 = pg.theta.clone()
        st = pg.run_episode(x0)
        torch.cuda.synchronize()
        if not graphs:
            _check_episode(pg, st, theta0, K, all_valid)
        runs.append([t.clone() for t in (pg.theta, pg.msg, pg.step_out, pg.delta, pg.S, pg.A, pg.C, pg.w)] + [torch.tensor(st.gn_info)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_policy_gradient_refuses_more_than_64_entries_and_no_exploration():
    with pytest.raises(ValueError, match="81"):
        _chain(learn=("Q",))
    with pytest.raises(ValueError, match="noise_scale"):
        from mpc4rl_amd import BatchedLinearSystemEnv, LinearPolicyGradient, linear_system_ocp
        LinearPolicyGradient(linear_system_ocp(), BatchedLinearSystemEnv(8, device=DEV, seed=5), 6, noise_scale=0.0)


def test_existing_learner_is_unchanged_beside_a_policy_gradient_learner():
    """A LinearQLearning episode at default settings is the same bits alone and after a policy-gradient learner was built and run beside
    it (the shared constructor and episode code take the same path for it)."""
    from mpc4rl_amd import BatchedLinearSystemEnv, LinearQLearning, linear_system_ocp

    def episode():
        ql = LinearQLearning(linear_system_ocp(), BatchedLinearSystemEnv(8, device=DEV, seed=5), 6)
        st = ql.run_episode()
        torch.cuda.synchronize()
        assert ql.sample_mpc.B == 8 * 5 and ql.msg.numel() == ql.n_p + 2
        return [t.clone() for t in (ql.theta, ql.msg, ql.step_out, ql.td, ql.valid, ql.S, ql.A, ql.C)] + [torch.tensor(st.total_cost)]

    alone = episode()
    pg, _ = _linear(lr=0.05)
    pg.run_episode()
    beside = episode()
    for a, b in zip(alone, beside):
        assert torch.equal(a, b)
