"""The binding read from include/mpcrl.h (mpc4rl_amd/_lib.py): the parser on literal snippets and on the real header, ProblemSpec's
field types, and what ``call`` refuses before anything reaches the library.  No GPU: the library loads, nothing below calls into it
except the argument refusals of host-only exports."""
import ctypes as C
import os
import re

import pytest
import torch

from test_cabi import ROOT, declared_symbols

from mpc4rl_amd import _lib
from mpc4rl_amd._lib import parse_header

CUDA0 = torch.device("cuda", 0)      # a device with an index: `call` then asks torch.cuda nothing before its checks


def functions(text):
    return parse_header(text).functions


# ---------------------------------------------------------------------- the parser on snippets
def test_scalars_and_return_types():
    f = functions("int mpcrl_a(int n, int64_t ld, double gamma);\nint64_t mpcrl_b_workspace_bytes(int T);")
    assert f == {"mpcrl_a": ("int", [("n", "int"), ("ld", "int64"), ("gamma", "double")]),
                 "mpcrl_b_workspace_bytes": ("int64", [("T", "int")])}


def test_handle_and_pointers_of_every_kind():
    f = functions("typedef struct MpcrlSolver *mpcrl_handle;\n"
                  "int mpcrl_a(mpcrl_handle h, double *a, float *b, int32_t *c, int64_t *d, uint8_t *e, void *f, void *stream);\n"
                  "int mpcrl_create(const MpcrlProblemSpec *spec, int batch, mpcrl_handle *out);")
    assert [k for _, k in f["mpcrl_a"][1]] == ["handle", "double*", "float*", "int32*", "int64*", "uint8*", "void*", "void*"]
    assert f["mpcrl_a"][1][-1] == ("stream", "void*")
    assert f["mpcrl_create"][1] == [("spec", "spec*"), ("batch", "int"), ("out", "handle*")]


def test_const_is_dropped_and_the_star_may_sit_anywhere():
    f = functions("int mpcrl_a(const double *x, const int32_t* idx, const uint8_t * live, double*out);")
    assert f["mpcrl_a"][1] == [("x", "double*"), ("idx", "int32*"), ("live", "uint8*"), ("out", "double*")]


def test_void_parameter_list():
    assert functions("int mpcrl_version(void);") == {"mpcrl_version": ("int", [])}


def test_prototype_over_several_lines_with_a_comment_inside():
    f = functions("int mpcrl_solve(mpcrl_handle h, const double *x0,\n"
                  "                int flags, uint8_t *active /* [K]: 0 free (1 at l), 2 at u */,\n"
                  "                void *stream);")
    assert f["mpcrl_solve"][1] == [("h", "handle"), ("x0", "double*"), ("flags", "int"), ("active", "uint8*"), ("stream", "void*")]


def test_array_parameter_is_a_pointer():
    assert functions("int mpcrl_plan(int model, int32_t out[12]);")["mpcrl_plan"][1] == [("model", "int"), ("out", "int32*")]
    assert functions("int mpcrl_plan(double par[]);")["mpcrl_plan"][1] == [("par", "double*")]


def test_comments_hold_no_exports():
    f = functions("/* use as  int mpcrl_foo(int x);  (or mpcrl_bar(h, flags, stream)) ... f(x) */\n"
                  "// int mpcrl_baz(int x);\n"
                  "int mpcrl_real(int x); /* mpcrl_tail(void); */")
    assert list(f) == ["mpcrl_real"]


@pytest.mark.parametrize("text", [
    "int mpcrl_a(size_t n);",                       # a type the binding does not know
    "int mpcrl_a(float x);",                        # float is known as a pointee only
    "int mpcrl_a(double **rows);",                  # no pointers to pointers
    "int mpcrl_a(struct Foo *p);",
    "int mpcrl_a(int);",                            # an unnamed parameter
    "float mpcrl_a(int n);",                        # a return type other than int / int64_t
    "int mpcrl_a(int (*callback)(int));",           # a prototype the pattern cannot take apart
    "enum { MPCRL_X = 1 << 2 };",                   # an enumerator that is no plain integer
])
def test_what_cannot_be_classified_raises(text):
    with pytest.raises(ValueError):
        parse_header(text)


def test_constants_and_struct_fields():
    h = parse_header("#ifndef MPCRL_H\n#define MPCRL_H\n#define MPCRL_ABI_VERSION 7\n#define MPCRL_NO_BOUND 1e30 /* absent */\n"
                     "enum { MPCRL_A = 0, MPCRL_B = 1 };\nenum {\n  MPCRL_F = 4, /* four (4) */\n  MPCRL_E_ARG = -1\n};\n"
                     "typedef struct {\n  int32_t nx, nu; /* sizes */\n  double dT;\n  const double *lb, *ub;\n  const int32_t *soft;\n} MpcrlProblemSpec;\n")
    assert h.constants == {"ABI_VERSION": 7, "NO_BOUND": 1e30, "A": 0, "B": 1, "F": 4, "E_ARG": -1}
    assert h.spec_fields == [("nx", "int32"), ("nu", "int32"), ("dT", "double"), ("lb", "double*"), ("ub", "double*"), ("soft", "int32*")]
    with pytest.raises(ValueError):
        parse_header("typedef struct { float x; } MpcrlProblemSpec;")


# ---------------------------------------------------------------------- the parser on include/mpcrl.h
def test_exports_are_the_declared_symbols():
    assert sorted(_lib.EXPORTS) == declared_symbols() and len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) == 68


def test_only_workspace_sizes_return_int64():
    for name, (ret, _) in _lib.HEADER.functions.items():
        assert ret == ("int64" if name.endswith("_workspace_bytes") or "_workspace_bytes_" in name else "int"), name
    assert sum(ret == "int64" for ret, _ in _lib.HEADER.functions.values()) == 9


D, F, I32, I64, U8, V = "double*", "float*", "int32*", "int64*", "uint8*", "void*"
WRITTEN_OUT = {
    "mpcrl_solve": ["handle", D, D, "int", D, D, D, D, I32, I32, V],
    "mpcrl_set_bounds": ["handle", "int", D, D],
    "mpcrl_env_chain_step": ["int", "double", "int", D, "int64", D, "int", D, D, D, "double", V, "int", D, V],
    "mpcrl_debug_launch_plan": ["int"] * 9 + [I32],
    "mpcrl_ppo_chain_collect": ["int", "double", "int", D, "int64", D, "double", "int", "int", "int", D, I64, D, I32, F, D, D, D, D, D, "double",
                                "int64", D, "double", D, D, D, D, D, D, D, U8, U8, U8, D, I32, V],
}


@pytest.mark.parametrize("name", sorted(WRITTEN_OUT))
def test_signatures_written_out_by_hand(name):
    kinds = [k for _, k in _lib.HEADER.functions[name][1]]
    assert kinds == WRITTEN_OUT[name]
    assert len(WRITTEN_OUT["mpcrl_solve"]) == 11 and len(WRITTEN_OUT["mpcrl_ppo_chain_collect"]) == 37


def test_constants_come_from_the_header():
    assert _lib.ABI_VERSION == 132 and _lib.NO_BOUND == 1e30
    assert (_lib.SENS_V, _lib.SENS_PI, _lib.RTI, _lib.COLD, _lib.COLD_DUAL, _lib.NO_BND_STORE, _lib.EXACT_QP) == (1, 2, 4, 8, 16, 32, 64)
    assert (_lib.MODEL_CARTPOLE, _lib.MODEL_LINEAR, _lib.MODEL_CHAIN, _lib.COST_NLS, _lib.COST_EXTERNAL) == (0, 1, 2, 0, 1)
    assert (_lib.BOUNDS_U0, _lib.BOUNDS_STAGE, _lib.BOUNDS_TERMINAL) == (0, 1, 2)
    assert (_lib.E_ARG, _lib.E_MODEL, _lib.E_HIP, _lib.E_NOMEM) == (-1, -2, -3, -4)


def test_problem_spec_field_types_match_the_header():
    """Independently of the parser: the struct's text, statement by statement."""
    hdr = open(os.path.join(ROOT, "include", "mpcrl.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct {") + len("typedef struct {"): hdr.index("} MpcrlProblemSpec;")], flags=re.S)
    ctype = {"int32_t": C.c_int32, "double": C.c_double, "const double *": C.POINTER(C.c_double), "const int32_t *": C.POINTER(C.c_int32)}
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        base = re.match(r"(const\s+)?\w+", stmt).group(0)
        for part in stmt[len(base):].split(","):
            part = part.strip()
            fields.append((part.lstrip("* "), ctype[base + " *" if part.startswith("*") else base]))
    assert fields == _lib.ProblemSpec._fields_ and len(fields) == 23
    assert [(n, _lib._FIELD[k]) for n, k in _lib.HEADER.spec_fields] == fields


# ---------------------------------------------------------------------- load() and call() without a GPU
def test_argtypes_and_restype_follow_the_parse():
    lib = _lib.load()
    ctype = {"int": C.c_int, "int64": C.c_int64, "double": C.c_double}
    for name, (ret, params) in _lib.HEADER.functions.items():
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret] and list(fn.argtypes) == [ctype.get(k, C.c_void_p) for _, k in params], name


def test_pointer_parameters_take_what_the_call_sites_pass():
    """ctypes arrays, POINTER(c_double) instances, byref(...), ints and None through c_void_p: mpcrl_debug_launch_plan (a pure host
    function) writes through each of them, and the NULL is refused by the library, not by ctypes."""
    lib = _lib.load()
    args = (_lib.MODEL_CARTPOLE, 20, 4096, 1024, 0, 0, 1, 3, 0)
    want = (C.c_int32 * 12)()
    assert lib.mpcrl_debug_launch_plan(*args, want) == 0 and _lib.call("mpcrl_debug_launch_plan", *args, want) == 0
    for how in (lambda a: C.cast(a, C.POINTER(C.c_int32)), lambda a: C.byref(a), lambda a: C.addressof(a), lambda a: C.c_void_p(C.addressof(a))):
        out = (C.c_int32 * 12)()
        assert _lib.call("mpcrl_debug_launch_plan", *args, how(out)) == 0 and list(out) == list(want)
    with pytest.raises(RuntimeError, match=r"mpcrl_debug_launch_plan failed with -1 \(MPCRL_E_ARG\)"):
        _lib.call("mpcrl_debug_launch_plan", *args, None)
    lo = (C.c_double * 1)(0.0)
    assert lib.mpcrl_set_bounds(None, 0, C.cast(lo, C.POINTER(C.c_double)), lo) == _lib.E_ARG      # (no handle: refused on the host)
    assert lib.mpcrl_get_launch_times(None, 0, C.byref(C.c_double()), C.byref(C.c_double())) == _lib.E_ARG


def test_call_refuses_a_wrong_argument_count():
    x = torch.zeros(3, 2, dtype=torch.float64)
    for args in ((x, 2, None, 3, 2), (x, 2, None, 3, 2, x, 0), (x, 2, None, 3, 2, x, None, None)):     # one short; the stream given; one more
        with pytest.raises(TypeError, match="mpcrl_weighted_grad_sum takes 6 arguments"):
            _lib.call("mpcrl_weighted_grad_sum", *args, device=CUDA0)
    with pytest.raises(TypeError, match="mpcrl_version takes 0 arguments"):
        _lib.call("mpcrl_version", 1)
    assert _lib.call("mpcrl_version") == 132


def test_call_refuses_a_tensor_for_a_scalar_or_a_handle():
    x = torch.zeros(3, 2, dtype=torch.float64)
    with pytest.raises(TypeError, match="mpcrl_weighted_grad_sum: parameter rows"):
        _lib.call("mpcrl_weighted_grad_sum", None, 2, None, torch.tensor(3), 2, None, device=CUDA0)
    with pytest.raises(TypeError, match="mpcrl_reset: parameter h "):
        _lib.call("mpcrl_reset", x, None, device=CUDA0)


def test_call_refuses_the_wrong_dtype():
    x = torch.zeros(3, 2, dtype=torch.float64)
    with pytest.raises(TypeError, match="mpcrl_weighted_grad_sum: parameter grad points to torch.float64, the tensor given holds torch.float32"):
        _lib.call("mpcrl_weighted_grad_sum", x.float(), 2, None, 3, 2, x, device=CUDA0)
    with pytest.raises(TypeError, match="mpcrl_set_order: parameter perm points to torch.int32"):
        _lib.call("mpcrl_set_order", None, torch.zeros(4, dtype=torch.int64), device=CUDA0)


def test_call_refuses_a_cpu_tensor():
    x = torch.zeros(3, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="mpcrl_weighted_grad_sum: the tensor given for grad lives on cpu"):
        _lib.call("mpcrl_weighted_grad_sum", x, 2, None, 3, 2, x, device=CUDA0)


def test_call_needs_a_device_where_the_export_takes_a_stream():
    with pytest.raises(TypeError, match="mpcrl_weighted_grad_sum launches on a stream"):
        _lib.call("mpcrl_weighted_grad_sum", None, 2, None, 3, 2, None)


def test_critic_td_grad_keeps_its_error_for_a_refused_shape():
    from mpc4rl_amd.td3 import critic_td_grad
    rows, a_next = torch.zeros(4, 2 * 40 + 30 + 2), torch.zeros(4, 30)
    with pytest.raises(ValueError, match="nx \\+ nu <= 64, n_critics 1 or 2"):       # refused by the size query, on the host
        critic_td_grad(rows, 40, 30, a_next, None, None, None, 2, 0.99, 1.0, None)
    with pytest.raises(ValueError, match="n_critics 1 or 2"):
        critic_td_grad(rows[:, :12], 4, 1, a_next[:, :1].contiguous(), None, None, None, 3, 0.99, 1.0, None)


def test_workspace_raises_on_a_refused_size():
    with pytest.raises(RuntimeError, match="mpcrl_cdpg_workspace_bytes failed with -1"):
        _lib.workspace("mpcrl_cdpg_workspace_bytes", 1, 4, 3, device="cpu")
    assert _lib.call("mpcrl_qlearning_td_workspace_bytes", 5, 4, 3) > 0
