"""The dynamics jets on the device, point by point, through the probe export mpcrl_debug_model_jets (jet_probe_kernel.hpp): the discrete
map of the cartpole and of the linear system evaluated with Jet1 / JetH / Jet2 seeded as the kernels seed them, against the 50-digit
reference of tests/model_jet_cases.py (held to numerical differentiation in tests/test_model_jets_cpu.py).

The bar is measured, not fixed: per block, err = max |dev - ref| / max |ref| at each point, and
    max over points err_dev <= 4 max(max over points err_float64, 2^-52),
err_float64 being the error of the same formulas in plain IEEE doubles (the yardstick).  fma contraction, the jets' reciprocal (about
1 ulp where a division is correctly rounded) and another association of the product rule each cost at most a doubling of the
per-operation rounding and do not all align: a factor 4.  The ratios measured are tabulated in DESIGN.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import model_jet_cases as S

pytestmark = pytest.mark.gpu

FACTOR = 4.0
SENTINEL = -12345.678
MODEL_ID = {"cartpole": 0, "linear": 1}      # MPCRL_MODEL_CARTPOLE, MPCRL_MODEL_LINEAR
E_ARG = -1


def _dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device="cuda:0").contiguous()      # (a copy: the case arrays are read-only)


def probe(cs, which, n=None):
    """One launch of form `which` over the first n points of the case set; returns [n + 1][row]: the rows and the sentinel row behind them"""
    from mpc4rl_amd import _lib
    from mpc4rl_amd.batch import _ptr
    lib = _lib.load()
    n = cs.n if n is None else n
    d = cs.dims
    x, u, th = _dev(cs.x[:n]), _dev(cs.u[:n]), _dev(cs.th[:n])
    aux = _dev(cs.nu[:n]) if which == 1 else _dev(cs.y[:n]) if which == 3 else None
    assert tuple(x.shape) == (n, d.nx) and tuple(u.shape) == (n, d.nu) and tuple(th.shape) == (n, d.ntd)
    assert aux is None or tuple(aux.shape) == (n, d.nx if which == 1 else d.nx + d.nu)
    out = torch.full((n + 1, S.row_size(cs.model, which)), SENTINEL, dtype=torch.float64, device="cuda:0")
    rc = lib.mpcrl_debug_model_jets(MODEL_ID[cs.model], which, n, cs.h, cs.rk_steps, _ptr(x), _ptr(u), _ptr(th),
                                    _ptr(aux) if aux is not None else None, _ptr(out), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def device_blocks(name):
    """{which: {block: [n][...]}} of the case set: one probe launch per form, shared by the tests"""
    cs = S.case_set(name)
    out = {}
    for which in range(4):
        rows = probe(cs, which)
        assert (rows[cs.n] == SENTINEL).all(), "the probe wrote behind its last row"
        out[which] = S.split_row(cs.model, which, rows[:cs.n])
    return out


@functools.lru_cache(maxsize=None)
def bar(name, block):
    """(4 max(yardstick error, 2^-52), yardstick error) of a block"""
    err, _ = S.block_errors(S.yardstick(name)[block], S.reference(name)[block])
    return FACTOR * max(float(err.max()), 2.0 ** -52), float(err.max())


def describe(cs, i):
    return f"point {i}: x = {cs.x[i].tolist()}, u = {cs.u[i].tolist()}, theta = {cs.th[i].tolist()}, h = {cs.h}, rk_steps = {cs.rk_steps}"


def check_block(name, label, block, got, failures):
    """got against the reference of `block`; prints the measured figures, appends a description of the worst point on failure"""
    cs, ref = S.case_set(name), S.reference(name)[block]
    err, diff = S.block_errors(got, ref)
    limit, yard = bar(name, block)
    i = int(err.argmax())
    print(f"[jets] {name:15s} {label:28s} {block:4s} err {err.max():.3e}  float64 {yard:.3e}  ratio to max(float64, 2^-52) "
          f"{err.max() / max(yard, 2.0 ** -52):.2f}")
    if not err.max() <= limit:
        e = np.unravel_index(int(diff[i].argmax()), diff[i].shape)
        failures.append(f"{name} {label} {block}: err {err.max():.3e} > {limit:.3e} at {describe(cs, i)}; entry {tuple(int(k) for k in e)}: "
                        f"device {np.asarray(got)[i][e]!r}, reference {ref[0][i][e]!r} + {ref[1][i][e]!r}")


@pytest.mark.parametrize("which", [0, 1, 2, 3])
@pytest.mark.parametrize("name", S.CASE_SETS)
def test_every_block_against_the_reference(name, which):
    dev = device_blocks(name)[which]
    failures = []
    for block in S.BLOCKS[which]:
        check_block(name, f"form {which}", block, dev[block], failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", S.CASE_SETS)
def test_forms_agree_with_each_other(name):
    """[B A] of Jet1 and JetH, dF/dtheta of Jet1 and Jet2, the inner tangent e against [B A] y, hdd against sum nu_m H_m: each pair within
    the bar of its block, measured as the blocks are (difference over the reference's largest entry at the point)."""
    cs, dev, ref = S.case_set(name), device_blocks(name), S.reference(name)
    failures = []

    def agree(label, block, a, b):
        n = cs.n
        scale = np.abs(ref[block][0]).reshape(n, -1).max(axis=1)
        scale = np.maximum(scale, scale.max() * 1e-300)
        worst = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).reshape(n, -1).max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.where(scale > 0, worst / scale, np.where(worst == 0, 0.0, np.inf))
        limit, yard = bar(name, block)
        print(f"[jets] {name:15s} {label:28s} {block:4s} differ {err.max():.3e}  ratio to max(float64, 2^-52) {err.max() / max(yard, 2.0 ** -52):.2f}")
        if not err.max() <= limit:
            failures.append(f"{name} {label}: {err.max():.3e} > {limit:.3e} at {describe(cs, int(err.argmax()))}")

    agree("BA form 0 / form 1", "BA", dev[0]["BA"], dev[1]["BA"])
    agree("Fth form 2 / g form 3", "Fth", dev[2]["Fth"], dev[3]["g"])
    ld = np.longdouble
    agree("e form 3 / BA y", "e", dev[3]["e"], np.einsum("nmj,nj->nm", dev[0]["BA"].astype(ld), cs.y.astype(ld)).astype(np.float64))
    agree("hdd / sum nu H", "hdd", dev[1]["hdd"], np.einsum("nm,nme->ne", cs.nu.astype(ld), dev[1]["H"].astype(ld)).astype(np.float64))
    assert not failures, "\n".join(failures)
    # the value of the map: the same bits from all four forms (DESIGN.md records that it is)
    for which in (1, 2, 3):
        same = np.array_equal(dev[0]["F"].view(np.int64), dev[which]["F"].view(np.int64))
        print(f"[jets] {name:15s} F form 0 / form {which} bit-identical: {same}")
        assert same, (name, which)


@pytest.mark.parametrize("name", ["cartpole", "cartpole_2step"])
def test_trivial_columns_are_exact_and_the_others_computed(name):
    """The columns of A for the cart position and velocity are e_0 and [h rk_steps, 1, 0, 0]' bit for bit (CartpoleDev::lin_trivial);
    the columns of u, theta, theta_dot are computed and agree with the reference."""
    cs, dev = S.case_set(name), device_blocks(name)
    e0 = np.array([1.0, 0.0, 0.0, 0.0])
    e1 = np.array([cs.h * cs.rk_steps, 1.0, 0.0, 0.0])
    failures = []
    for which in (0, 1):
        BA = dev[which]["BA"]
        assert np.array_equal(BA[:, :, 1].view(np.int64), np.broadcast_to(e0, (cs.n, 4)).copy().view(np.int64)), which
        assert np.array_equal(BA[:, :, 2].view(np.int64), np.broadcast_to(e1, (cs.n, 4)).copy().view(np.int64)), which
        _, diff = S.block_errors(BA, S.reference(name)["BA"])
        scale = np.abs(S.reference(name)["BA"][0]).reshape(cs.n, -1).max(axis=1)       # the block's largest entry at the point, as in the block test
        limit, _ = bar(name, "BA")
        for col, what in ((0, "u"), (3, "theta"), (4, "theta_dot")):
            err = diff[:, :, col].max(axis=1) / scale
            print(f"[jets] {name:15s} form {which} column {what:9s} err {err.max():.3e}")
            if not err.max() <= limit:
                failures.append(f"{name} form {which} column {what}: {err.max():.3e} > {limit:.3e} at {describe(cs, int(err.argmax()))}")
    assert not failures, "\n".join(failures)


def test_jet_rcp_is_within_one_ulp():
    """jet_rcp (hardware seed and two Newton steps; jet.hpp documents "~1 ulp") against the correctly rounded 1 / x of mpmath"""
    from mpc4rl_amd import _lib
    from mpc4rl_amd.batch import _ptr
    lib = _lib.load()
    x = S.rcp_inputs()
    xd = _dev(x)
    out = torch.full((x.size + 1,), SENTINEL, dtype=torch.float64, device="cuda:0")
    assert lib.mpcrl_debug_model_jets(0, 4, x.size, 0.0, 0, _ptr(xd), None, None, None, _ptr(out), None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[-1] == SENTINEL
    err = S.rcp_ulp_errors(x, got[:-1])
    i = int(err.argmax())
    exact = np.array([float(1 / S.mpf(float(a))) for a in x])
    print(f"[jets] jet_rcp: max error {err.max():.4f} ulp at x = {x[i]!r}; {int((got[:-1] != exact).sum())} of {x.size} not correctly rounded")
    assert err.max() <= 1.0, (err.max(), x[i], got[i])
    pw = np.abs(np.frexp(x)[0]) == 0.5
    assert np.array_equal(got[:-1][pw], 1.0 / x[pw])        # a power of two has an exact reciprocal


def test_probe_refuses_bad_arguments():
    from mpc4rl_amd import _lib
    from mpc4rl_amd.batch import _ptr
    lib = _lib.load()
    inp = torch.ones(64, dtype=torch.float64, device="cuda:0")          # 3 points of at most 8 doubles
    res = torch.zeros(1024, dtype=torch.float64, device="cuda:0")       # 3 rows of at most 54 doubles
    p, q = _ptr(inp), _ptr(res)
    call = lambda model=0, which=1, n=3, h=0.025, rk=1, x=p, u=p, th=p, aux=p, out=q: \
        lib.mpcrl_debug_model_jets(model, which, n, h, rk, x, u, th, aux, out, None)
    assert call() == 0 and call(model=1, rk=0) == 0 and call(which=0, aux=None) == 0 and call(which=2, aux=None) == 0
    for kw in (dict(x=None), dict(u=None), dict(th=None), dict(aux=None), dict(which=3, aux=None), dict(out=None),
               dict(which=4, x=None), dict(which=4, out=None),
               dict(n=0), dict(n=-1), dict(which=4, n=0), dict(which=-1), dict(which=5),
               dict(rk=0), dict(rk=5), dict(rk=-1), dict(model=2), dict(model=3), dict(model=-1)):
        assert call(**kw) == E_ARG, kw
    host = (C.c_double * 64)()
    assert call(x=C.cast(host, C.c_void_p)) == E_ARG
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", S.CASE_SETS)
def test_rows_do_not_depend_on_the_launch_size(name):
    """n = 1 (one lane of one workgroup) and n = 67 (a full and a partial workgroup): the row behind the last one keeps its sentinel,
    and the rows the two launches share are the same bits"""
    cs = S.case_set(name)
    for which in range(4):
        one, full = probe(cs, which, n=1), probe(cs, which, n=cs.n)
        for rows, n in ((one, 1), (full, cs.n)):
            assert (rows[n] == SENTINEL).all(), (name, which, n)
            assert not (rows[:n] == SENTINEL).any(), (name, which, n)
        assert np.array_equal(one[:1].view(np.int64), full[:1].view(np.int64)), (name, which)
        blocks = S.split_row(cs.model, which, full[:cs.n])
        for b, v in device_blocks(name)[which].items():
            assert np.array_equal(v.view(np.int64), blocks[b].view(np.int64)), (name, which, b)
