"""GPU tests of the Q-learners' Gauss-Newton step (csrc/qlearning_gn_kernel.hpp): mpcrl_qlearning_td_gn against its torch statement
``qlearning_gn_terms`` on synthetic tables and bit for bit against mpcrl_qlearning_td_grad, mpcrl_qlearning_gn_apply against
``qlearning_gn_step`` and ``np.linalg.solve``, and LinearQLearning / ChainQLearning with method="gauss_newton" end to end, eager and
replayed from graphs.

Bounds (derived, not measured), eps = 2^-53:
  sums   |G_ac - G_ref,ac| <= 4 M eps sum_j |g_ja g_jc| over the M terms (any summation order), likewise b with |td_j g_ja|;
  solve  ||d - d_ref||_2 <= 8 K (K + 1) eps cond_2(H) ||d_ref||_2 (backward stability of Cholesky, on both sides), cond_2 of the H the test
         built.
Every comparison prints its observed figure beside the bound."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)
EPS = 2.0 ** -53
POISON = -7.0


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _lib():
    from mpc4rl_amd import _lib
    return _lib.load()


def make_table(T, E, n_p, idx, seed, all_invalid=False):
    """An episode table (CPU tensors) with every kind of term: live columns that end after 1 and after 2 rows (and other lengths), failed
    Q and V solves with NaN in their Q, V and dQ, NaN in the rows of dead environments, and one NaN inside a valid row's unlearned
    column.  Environment 2 is all valid."""
    rng = np.random.default_rng(seed)
    L = rng.integers(3, T + 1, E)
    L[rng.uniform(size=E) < 0.8] = T
    L[0], L[1], L[2] = 1, 2, T
    if all_invalid:
        L[:] = 2
    live = (np.arange(T)[:, None] < L[None, :]).astype(np.uint8)
    cost = rng.uniform(0, 5, (T, E)) * live
    q, v = rng.normal(size=(T - 1, E)), rng.normal(size=(T - 1, E))
    dq = rng.normal(size=(T - 1, E, n_p)) * 10.0 ** rng.integers(-2, 3, n_p)
    sq = np.where(rng.uniform(size=(T - 1, E)) < 0.1, 2, 0).astype(np.int32)
    sv = np.where(rng.uniform(size=(T - 1, E)) < 0.05, 4, 0).astype(np.int32)
    sq[:, 2], sv[:, 2] = 0, 0
    q[sq != 0], v[sv != 0], dq[sq != 0] = np.nan, np.nan, np.nan
    dead = live[: T - 1] == 0
    q[dead], v[dead], dq[dead] = np.nan, np.nan, np.nan
    free = [c for c in range(n_p) if c not in set(idx)]
    if free and not all_invalid:
        dq[0, 2, free[0]] = np.nan                                  # valid row, unlearned column: never read
    return [torch.as_tensor(a) for a in (q, v, dq, sq, sv, cost, live)]


def run_td_gn(d, T, E, n_p, gamma, idx, launches=1):
    """mpcrl_qlearning_td_gn on the table d (CPU tensors): (msg, td, valid) of every launch, as CPU tensors."""
    lib = _lib()
    K = len(idx)
    dev = [t.to(DEV).contiguous() for t in d]
    idx_d = torch.tensor(idx, dtype=torch.int32, device=DEV)
    nb = lib.mpcrl_qlearning_gn_workspace_bytes(T, E, K)
    assert nb > 0
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    out = []
    for _ in range(launches):
        msg = torch.full((K * (K + 1) // 2 + K + 2,), POISON, **F64)
        td = torch.full((T - 2, E), POISON, **F64)
        valid = torch.full((T - 2, E), 9, dtype=torch.uint8, device=DEV)
        assert lib.mpcrl_qlearning_td_gn(*[_p(t) for t in dev], T, E, n_p, gamma, _p(idx_d), K, _p(ws), _p(td), _p(valid), _p(msg), _stream()) == 0
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32)[0]) == 0                # the ticket is left zero
        out.append((msg.cpu(), td.cpu(), valid.cpu()))
    return out


def sum_bounds(d, valid, td, idx, M):
    """4 M eps sum_j |g_ja g_jc| in the message's packing, then 4 M eps sum_j |td_j g_ja|, sum |td_j|, and 0 for the count."""
    K = len(idx)
    g = torch.nan_to_num(d[2][: valid.shape[0]][..., idx]).abs()
    g = torch.where(valid[..., None], g, torch.zeros_like(g)).reshape(-1, K)
    t = td.abs().reshape(-1)
    iu = torch.triu_indices(K, K)
    return 4 * M * EPS * torch.cat([(g.t() @ g)[iu[0], iu[1]], g.t() @ t, t.sum().reshape(1), torch.zeros(1, dtype=torch.float64)])


def check_message(got, d, gamma, idx, M, what):
    from mpc4rl_amd import qlearning_gn_terms
    msg, td, valid = qlearning_gn_terms(*d, gamma, idx)
    bound = sum_bounds(d, valid, td, idx, M)
    assert torch.isfinite(got[0]).all()
    assert torch.equal(got[1], td) and torch.equal(got[2].bool(), valid), what
    assert float(got[0][-1]) == float(valid.sum())
    diff = (got[0] - msg).abs()
    worst = float((diff / bound.clamp(min=1e-300))[:-1].max())
    print(f"{what}: count {int(valid.sum())} of {M}, largest difference / bound {worst:.3e}")
    assert bool((diff <= bound).all()), what
    return msg, td, valid


def _idx(K, spread):
    return list(range(K)) if not spread else [3 * a + 1 for a in range(K)]


@pytest.mark.parametrize("spread", [False, True], ids=["np=K", "np=3K+1"])
@pytest.mark.parametrize("K", [1, 3, 16, 17, 40, 64])
@pytest.mark.parametrize("T,E", [(3, 5), (5, 43), (12, 128)])
def test_td_gn_kernel_matches_torch_form(T, E, K, spread):
    """3 x 5: 5 terms; 5 x 43: 129 terms, one block plus one term; 12 x 128: 10 blocks (the four slices of the final sum).  Two launches
    give the same bits; td and valid are mpcrl_qlearning_td_grad's bits."""
    lib = _lib()
    n_p, idx, gamma = (3 * K + 1 if spread else K), _idx(K, spread), 0.97
    M = (T - 2) * E
    d = make_table(T, E, n_p, idx, 100 * T + K)
    first, second = run_td_gn(d, T, E, n_p, gamma, idx, launches=2)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    _, td, valid = check_message(first, d, gamma, idx, M, f"T {T} E {E} K {K} n_p {n_p}")
    assert 0 < int(valid.sum()) < M
    # the first-order kernel on the same inputs
    dev = [t.to(DEV).contiguous() for t in d]
    ws = torch.zeros(lib.mpcrl_qlearning_td_workspace_bytes(T, E, n_p), dtype=torch.uint8, device=DEV)
    td1, valid1, msg1 = torch.full((T - 2, E), POISON, **F64), torch.zeros(T - 2, E, dtype=torch.uint8, device=DEV), torch.zeros(n_p + 2, **F64)
    assert lib.mpcrl_qlearning_td_grad(*[_p(t) for t in dev], T, E, n_p, gamma, 1e-3, _p(ws), _p(td1), _p(valid1), _p(msg1), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(td1.cpu(), first[1]) and torch.equal(valid1.cpu(), first[2])


def test_td_gn_all_invalid_table_leaves_theta():
    lib = _lib()
    T, E, K, n_p, gamma = 5, 43, 3, 10, 0.97
    idx = _idx(K, True)
    d = make_table(T, E, n_p, idx, 1, all_invalid=True)
    (msg, td, valid), = run_td_gn(d, T, E, n_p, gamma, idx)
    assert float(msg.abs().sum()) == 0.0 and float(td.abs().sum()) == 0.0 and int(valid.sum()) == 0
    theta = torch.randn(n_p, generator=torch.Generator().manual_seed(0), dtype=torch.float64).to(DEV)
    theta0, step, info = theta.clone(), torch.full((n_p,), POISON, **F64), torch.full((1,), 7, dtype=torch.int32, device=DEV)
    idx_d = torch.tensor(idx, dtype=torch.int32, device=DEV)
    assert lib.mpcrl_qlearning_gn_apply(_p(msg.to(DEV)), K, _p(idx_d), n_p, 0.5, 1e-3, _p(theta), _p(step), _p(info), _stream()) == 0
    torch.cuda.synchronize()
    assert int(info) == -1 and torch.equal(theta, theta0) and float(step.abs().sum()) == 0.0


def test_td_gn_argument_checks():
    lib = _lib()
    T, E, n_p = 4, 3, 70
    z = torch.zeros(8, **F64)
    idx_d = torch.arange(65, dtype=torch.int32, device=DEV)
    for K in (0, 65, -1):
        assert lib.mpcrl_qlearning_gn_workspace_bytes(T, E, K) == -1
        assert lib.mpcrl_qlearning_td_gn(*[_p(z)] * 7, T, E, n_p, 0.9, _p(idx_d), K, _p(z), _p(z), None, _p(z), _stream()) == -1
        assert lib.mpcrl_qlearning_gn_apply(_p(z), K, _p(idx_d), n_p, 1.0, 0.0, _p(z), _p(z), _p(idx_d), _stream()) == -1
    assert lib.mpcrl_qlearning_td_gn(*[_p(z)] * 7, T, E, 2, 0.9, _p(idx_d), 3, _p(z), _p(z), None, _p(z), _stream()) == -1     # K > n_p
    assert lib.mpcrl_qlearning_td_gn(*[_p(z)] * 7, T, E, n_p, 0.9, None, 3, _p(z), _p(z), None, _p(z), _stream()) == -1
    assert lib.mpcrl_qlearning_gn_apply(_p(z), 3, _p(idx_d), n_p, 1.0, -1.0, _p(z), _p(z), _p(idx_d), _stream()) == -1
    m0 = torch.full((3 * 4 // 2 + 3 + 2,), POISON, **F64)                       # T = 2: no term, an empty message
    assert lib.mpcrl_qlearning_td_gn(*[None] * 7, 2, E, n_p, 0.9, _p(idx_d), 3, None, None, None, _p(m0), _stream()) == 0
    torch.cuda.synchronize()
    assert float(m0.abs().sum()) == 0.0


# ---------------------------------------------------------------------- the apply kernel
def run_apply(G, b, count, idx, n_theta, lr, damping):
    lib = _lib()
    K = len(idx)
    iu = np.triu_indices(K)
    msg = torch.as_tensor(np.concatenate([G[iu], b, [0.0], [float(count)]]))
    theta0 = torch.randn(n_theta, generator=torch.Generator().manual_seed(K), dtype=torch.float64)
    theta, step = theta0.to(DEV), torch.full((n_theta,), POISON, **F64)
    info = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    idx_d = torch.tensor(idx, dtype=torch.int32, device=DEV)
    assert lib.mpcrl_qlearning_gn_apply(_p(msg.to(DEV)), K, _p(idx_d), n_theta, lr, damping, _p(theta), _p(step), _p(info), _stream()) == 0
    torch.cuda.synchronize()
    step, theta = step.cpu(), theta.cpu()
    off = torch.ones(n_theta, dtype=torch.bool)
    off[idx] = False
    assert float(step[off].abs().sum()) == 0.0 and torch.equal(theta[off], theta0[off])          # only theta[idx] may move
    assert torch.equal(theta[idx], theta0[idx] + step[idx])
    return msg, step[idx], int(info)


@pytest.mark.parametrize("kappa", [1e2, 1e6])
@pytest.mark.parametrize("K", [1, 2, 17, 64])
def test_gn_apply_matches_solve(K, kappa):
    """H = Q diag(ev) Q' with cond_2 = kappa (K = 1: a scalar), count 37, without damping (H is then what the kernel factors) and with."""
    from mpc4rl_amd import qlearning_gn_step
    rng = np.random.default_rng(K)
    Qm = np.linalg.qr(rng.normal(size=(K, K)))[0]
    ev = np.logspace(0, -np.log10(kappa), K) if K > 1 else np.array([0.3])
    H = (Qm * ev) @ Qm.T
    H = 0.5 * (H + H.T)
    n, lr = 37, 0.8
    b = rng.normal(size=K)
    idx, n_theta = _idx(K, True), 3 * K + 5
    for damping in (0.0, 1e-3):
        msg, delta, info = run_apply(H * n, b * n, n, idx, n_theta, lr, damping)
        Gb = np.triu(H) + np.triu(H, 1).T                                   # what the message carries: the upper triangle
        Hd = Gb + damping * np.diag(np.diag(Gb))
        ref = lr * np.linalg.solve(Hd, b)
        bound = 8 * K * (K + 1) * EPS * np.linalg.cond(Hd) * np.linalg.norm(ref)
        torch_form, info_t = qlearning_gn_step(msg, K, lr, damping)
        e_np, e_t = np.linalg.norm(delta.numpy() - ref), np.linalg.norm(delta.numpy() - torch_form.numpy())
        print(f"K {K} kappa {kappa:g} damping {damping:g}: vs numpy {e_np:.3e}, vs torch form {e_t:.3e}, bound {bound:.3e}")
        assert info == 0 and info_t == 0
        assert e_np <= bound and e_t <= bound


def test_gn_apply_singular_and_damped():
    from mpc4rl_amd import qlearning_gn_step
    rng = np.random.default_rng(0)
    K, M = 5, 40
    g = rng.normal(size=(M, K))
    g[:, 3] = 0.0                                                   # an entry no term is sensitive to: G has a zero row and column
    td = rng.normal(size=M)
    G, b = g.T @ g, g.T @ td
    idx, n_theta = _idx(K, True), 3 * K + 5
    msg, delta, info = run_apply(G, b, M, idx, n_theta, 1.0, 0.0)
    assert info == 4 == qlearning_gn_step(msg, K, 1.0, 0.0)[1] and float(delta.abs().sum()) == 0.0
    msg, delta, info = run_apply(G, b, M, idx, n_theta, 1.0, 1e-3)
    ref, info_t = qlearning_gn_step(msg, K, 1.0, 1e-3)
    d = np.diag(G / M)
    Hd = G / M + 1e-3 * np.diag(np.where(d > 0, d, 1e-12 * d.max()))
    assert info == 0 == info_t and float(delta[3]) == 0.0
    assert np.linalg.norm(delta.numpy() - ref.numpy()) <= 8 * K * (K + 1) * EPS * np.linalg.cond(Hd) * np.linalg.norm(ref.numpy())
    for bad in (np.zeros((K, K)), np.where(np.eye(K) > 0, np.nan, G)):                      # d_max 0 / not finite
        _, delta, info = run_apply(bad, b, M, idx, n_theta, 1.0, 1e-3)
        assert info == -1 and float(delta.abs().sum()) == 0.0


# ---------------------------------------------------------------------- the loops
def _linear(graphs=False, **kw):
    from mpc4rl_amd import BatchedLinearSystemEnv, LinearQLearning, linear_system_ocp
    ql = LinearQLearning(linear_system_ocp(), BatchedLinearSystemEnv(8, device=DEV, seed=5), 6, noise_scale=0.1, seed=6, **kw)
    if graphs:
        ql.enable_graphs()
    return ql


def _chain(graphs=False, **kw):
    from mpc4rl_amd import BatchedChainMassEnv, ChainQLearning, chain_mass_ocp
    from mpc4rl_amd.problems import chain_param_layout
    ocp = chain_mass_ocp(3, N=10)
    off = chain_param_layout(3)[4]
    p = torch.tensor(ocp.p0)
    p[off["m"][0]: off["m"][1]] *= 1.1
    p[off["D"][0]: off["D"][1]] *= 0.9
    env = BatchedChainMassEnv(4, ocp, device=DEV, p=p, w_std=0.01, vel_std=1e-2, seed=1)
    ql = ChainQLearning(ocp, env, 4, noise_scale=0.05, seed=2, **kw)
    if graphs:
        ql.enable_graphs()
    return ql


def _check_gn_episode(ql, st, theta0, K_want):
    from mpc4rl_amd import qlearning_gn_step
    T, E, n = ql.T, ql.E, ql.T - 1
    rq, rv = ql.last_sweep
    idx = ql.learn_idx.cpu().tolist()
    assert len(idx) == ql.K == K_want and idx == torch.nonzero(ql.learn_mask.cpu()).reshape(-1).tolist()
    d = [rq.V.reshape(n, E).cpu(), rv.V.reshape(n, E).cpu(), rq.dV_dp.reshape(n, E, -1).cpu(), rq.status.reshape(n, E).cpu(),
         rv.status.reshape(n, E).cpu(), ql.C.cpu(), ql.live.cpu()]
    M = (T - 2) * E
    msg, td, valid = check_message((ql.msg.cpu(), ql.td.cpu(), ql.valid.cpu()), d, ql.gamma, idx, M, type(ql).__name__)
    assert int(valid.sum()) == M                                                  # no instance is left out
    # the solve, on the message the device holds: only the factorisation differs
    ref, info = qlearning_gn_step(ql.msg.cpu(), ql.K, ql.lr, ql.damping)
    KK = ql.K * (ql.K + 1) // 2
    Gb = np.zeros((ql.K, ql.K))
    Gb[np.triu_indices(ql.K)] = ql.msg.cpu().numpy()[:KK] / M
    Gb = Gb + np.triu(Gb, 1).T
    dg = np.diag(Gb)
    Hd = Gb + ql.damping * np.diag(np.where(dg > 0, dg, 1e-12 * dg.max()))
    step = ql.step_out.cpu()
    err, bound = float((step[idx] - ref).norm()), 8 * ql.K * (ql.K + 1) * EPS * np.linalg.cond(Hd) * float(ref.norm())
    print(f"{type(ql).__name__}: K {ql.K}, info {st.gn_info}, |step| {float(step.norm()):.3e}, step difference {err:.3e}, bound {bound:.3e}")
    assert st.gn_info == 0 == info and float(ref.norm()) > 0.0
    assert err <= bound
    off = torch.ones(ql.n_p, dtype=torch.bool)
    off[idx] = False
    assert float(step[off].abs().sum()) == 0.0 and torch.equal(st.step, ql.step_out)
    assert torch.equal(ql.theta, theta0 + ql.step_out)
    assert torch.equal(ql.rollout_mpc.get_theta(), ql.theta) and torch.equal(ql.sample_mpc.get_theta(), ql.theta)


@pytest.mark.parametrize("make,K", [(_linear, 12), (_chain, 20)], ids=["linear", "chain"])
def test_gauss_newton_episode_eager_and_from_graphs(make, K):
    """One episode with method="gauss_newton": the message against qlearning_gn_terms on the learner's own sweep, the applied step against
    qlearning_gn_step; the same episode replayed from graphs, from the same seeds, is the same bits."""
    runs = []
    for graphs in (False, True):
        ql = make(graphs=graphs, method="gauss_newton", lr=0.5, damping=1e-3)
        theta0 = ql.theta.clone()
        st = ql.run_episode()
        torch.cuda.synchronize()
        if not graphs:
            _check_gn_episode(ql, st, theta0, K)
        runs.append([t.clone() for t in (ql.theta, ql.msg, ql.step_out, ql.td, ql.S, ql.A, ql.C)] + [torch.tensor(st.gn_info)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_gauss_newton_refuses_more_than_64_entries():
    with pytest.raises(ValueError, match="81"):
        ql = _chain(method="gauss_newton", learn=("Q",))
        ql.run_episode()


def test_gradient_method_is_the_default_bit_for_bit():
    runs = []
    for kw in (dict(), dict(method="gradient", damping=0.5)):
        ql = _linear(lr=1e-3, **kw)
        st = ql.run_episode()
        torch.cuda.synchronize()
        assert st.gn_info == 0 and ql.msg.numel() == ql.n_p + 2
        runs.append([t.clone() for t in (ql.theta, ql.msg, ql.step_out, ql.td)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
