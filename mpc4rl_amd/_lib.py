"""ctypes binding of libmpcrl_hip.so, read from include/mpcrl.h (and include/mpcrl_ext.h, include/mpcrl_chain_ext.h, include/mpcrl_traj_ext.h, include/mpcrl_chain_traj_ext.h, include/mpcrl_bound_ext.h, include/mpcrl_cost_ext.h, include/mpcrl_traj_jvp_ext.h, include/mpcrl_chain_traj_jvp_ext.h, include/mpcrl_probe_ext.h and include/mpcrl_probe_chain_ext.h, a table of its own each), and the one path the package calls the library through
(``call``, ``workspace``).  Fails loudly when the library is missing.

The .hip units include the same header, so the compiler holds the implementation to it; the prototypes, constants and error codes here
are parsed from it, so the binding cannot disagree with either.  ``ProblemSpec`` alone is written by hand (its fields take typed
pointers) and is compared with the header's struct when the module is imported.

The header is read and parsed when this module is imported, not at ``load()``: the constants below are module attributes that other
modules and tests read without loading the library.  That needs the standard library only (torch and the library come with ``load()``),
and it means ``import mpc4rl_amd`` needs include/mpcrl.h beside the package; without it the import fails with a message saying so."""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List, NamedTuple, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPCRL_LIB_PATH") or os.path.join(_HERE, "libmpcrl_hip.so")   # the override is for instrumented builds (profiles/microbench)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpcrl.h")
EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpcrl_ext.h")   # extensions beyond the reference's MPC surface, versioned on their own

# ---------------------------------------------------------------------- the header, parsed (standard library only)
# parameter kinds: "int", "int64", "double", "handle"; pointers "double*", "float*", "int32*", "int64*", "uint8*", "void*", "spec*", "handle*"
_SCALAR = {"int": "int", "int64_t": "int64", "double": "double", "mpcrl_handle": "handle"}
_POINTEE = {"double": "double*", "float": "float*", "int32_t": "int32*", "int64_t": "int64*", "uint8_t": "uint8*", "void": "void*",
            "MpcrlProblemSpec": "spec*", "mpcrl_handle": "handle*"}
_RETURN = {"int": "int", "int64_t": "int64"}


class Header(NamedTuple):
    functions: Dict[str, Tuple[str, List[Tuple[str, str]]]]    # export -> (return kind, [(parameter name, kind)]), in header order
    constants: Dict[str, float]                                 # #defines and enumerators, without the MPCRL_ prefix
    spec_fields: List[Tuple[str, str]]                          # MpcrlProblemSpec: (field name, "int32" | "double" | "int32*" | "double*")


def _parameter(decl: str, where: str) -> Tuple[str, str]:
    m = re.fullmatch(r"(?:const\s+)?(\w+)(?:\s+|\s*(\*)\s*)(\w+)\s*(\[\s*\d*\s*\])?", decl.strip())
    if not m or (m.group(2) and m.group(4)):
        raise ValueError(f"{where}: cannot read the parameter {decl.strip()!r}")
    base, star, name, array = m.groups()
    kinds = _POINTEE if star or array else _SCALAR      # (a parameter declared as an array is a pointer)
    if base not in kinds:
        raise ValueError(f"{where}: parameter {name!r} has a type this binding does not know: {decl.strip()!r}")
    return name, kinds[base]


def parse_header(text: str) -> Header:
    """Every ``mpcrl_*`` prototype, ``MPCRL_*`` #define with a value and enumerator, and the fields of MpcrlProblemSpec.  Raises
    ValueError on a prototype, parameter or enumerator it cannot classify: nothing defaults to a pointer."""
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    functions = {}
    for ret, name, params in re.findall(r"\b(\w+)\s+(mpcrl_\w+)\s*\(([^()]*)\)\s*;", text):
        if ret not in _RETURN:
            raise ValueError(f"{name}: return type {ret!r} is neither int nor int64_t")
        params = [] if params.strip() == "void" else [_parameter(p, name) for p in params.split(",")]
        functions[name] = (_RETURN[ret], params)
    stray = set(re.findall(r"\b(mpcrl_\w+)\s*\(", text)) - set(functions)
    if stray:
        raise ValueError(f"cannot read the prototype of {', '.join(sorted(stray))}")
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+MPCRL_(\w+)[ \t]+(\S+)[ \t]*$", text, flags=re.M):
        constants[name] = float(value) if re.search(r"[.eE]", value) else int(value, 0)
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        for item in filter(None, (s.strip() for s in body.split(","))):
            m = re.fullmatch(r"MPCRL_(\w+)\s*=\s*(-?\d+)", item)
            if not m:
                raise ValueError(f"cannot read the enumerator {item!r}")
            constants[m.group(1)] = int(m.group(2))
    spec_fields = []
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*MpcrlProblemSpec\s*;", text)
    for decl in filter(None, (s.strip() for s in m.group(1).split(";"))) if m else ():
        f = re.fullmatch(r"(?:const\s+)?(int32_t|double)\b(.*)", decl, flags=re.S)
        names = [re.fullmatch(r"\s*(\*?)\s*(\w+)\s*", d) for d in f.group(2).split(",")] if f else [None]
        if not all(names):
            raise ValueError(f"MpcrlProblemSpec: cannot read the field {decl!r}")
        spec_fields += [(n.group(2), f.group(1).replace("_t", "") + n.group(1)) for n in names]
    return Header(functions, constants, spec_fields)


if not os.path.exists(HEADER_PATH):
    raise ImportError(f"mpc4rl_amd: {HEADER_PATH} not found. The binding is read from the header: keep include/ beside the package "
                      "(the repository's layout).")
with open(HEADER_PATH) as _f:
    HEADER = parse_header(_f.read())
EXPORTS = list(HEADER.functions)
if not os.path.exists(EXT_HEADER_PATH):
    raise ImportError(f"mpc4rl_amd: {EXT_HEADER_PATH} not found. The binding is read from the headers: keep include/ beside the package.")
with open(EXT_HEADER_PATH) as _f:
    EXT_HEADER = parse_header(_f.read())      # a table of its own: HEADER, EXPORTS and the constants below describe mpcrl.h alone
EXT_EXPORTS = list(EXT_HEADER.functions)
EXT_VERSION = EXT_HEADER.constants["EXT_VERSION"]
STATE_Q_MODE = EXT_HEADER.constants["STATE_Q_MODE"]
CHAIN_EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpcrl_chain_ext.h")   # du0*/dx0 of the chain of masses, versioned on its own
if not os.path.exists(CHAIN_EXT_HEADER_PATH):
    raise ImportError(f"mpc4rl_amd: {CHAIN_EXT_HEADER_PATH} not found. The binding is read from the headers: keep include/ beside the package.")
with open(CHAIN_EXT_HEADER_PATH) as _f:
    CHAIN_EXT_HEADER = parse_header(_f.read())      # a third table (the #include of mpcrl_ext.h is not followed)
CHAIN_EXT_EXPORTS = list(CHAIN_EXT_HEADER.functions)
CHAIN_EXT_VERSION = CHAIN_EXT_HEADER.constants["CHAIN_EXT_VERSION"]
TRAJ_EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpcrl_traj_ext.h")   # the trajectory vector-Jacobian product, versioned on its own
if not os.path.exists(TRAJ_EXT_HEADER_PATH):
    raise ImportError(f"mpc4rl_amd: {TRAJ_EXT_HEADER_PATH} not found. The binding is read from the headers: keep include/ beside the package.")
with open(TRAJ_EXT_HEADER_PATH) as _f:
    TRAJ_EXT_HEADER = parse_header(_f.read())      # a fourth table (the #include of mpcrl_ext.h is not followed)
TRAJ_EXT_EXPORTS = list(TRAJ_EXT_HEADER.functions)
TRAJ_EXT_VERSION = TRAJ_EXT_HEADER.constants["TRAJ_EXT_VERSION"]
CHAIN_TRAJ_EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpcrl_chain_traj_ext.h")   # the trajectory VJP of the chain of masses, versioned on its own
if not os.path.exists(CHAIN_TRAJ_EXT_HEADER_PATH):
    raise ImportError(f"mpc4rl_amd: {CHAIN_TRAJ_EXT_HEADER_PATH} not found. The binding is read from the headers: keep include/ beside the package.")
with open(CHAIN_TRAJ_EXT_HEADER_PATH) as _f:
    CHAIN_TRAJ_EXT_HEADER = parse_header(_f.read())      # a fifth table (the #include of mpcrl_ext.h is not followed)
CHAIN_TRAJ_EXT_EXPORTS = list(CHAIN_TRAJ_EXT_HEADER.functions)
CHAIN_TRAJ_EXT_VERSION = CHAIN_TRAJ_EXT_HEADER.constants["CHAIN_TRAJ_EXT_VERSION"]
BOUND_EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpcrl_bound_ext.h")   # the derivatives with respect to the box bounds, versioned on their own
if not os.path.exists(BOUND_EXT_HEADER_PATH):
    raise ImportError(f"mpc4rl_amd: {BOUND_EXT_HEADER_PATH} not found. The binding is read from the headers: keep include/ beside the package.")
with open(BOUND_EXT_HEADER_PATH) as _f:
    BOUND_EXT_HEADER = parse_header(_f.read())      # a sixth table (the #include of mpcrl_ext.h is not followed)
BOUND_EXT_EXPORTS = list(BOUND_EXT_HEADER.functions)
BOUND_EXT_VERSION = BOUND_EXT_HEADER.constants["BOUND_EXT_VERSION"]
COST_EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpcrl_cost_ext.h")   # the derivatives with respect to the cartpole's tracking cost, versioned on their own
if not os.path.exists(COST_EXT_HEADER_PATH):
    raise ImportError(f"mpc4rl_amd: {COST_EXT_HEADER_PATH} not found. The binding is read from the headers: keep include/ beside the package.")
with open(COST_EXT_HEADER_PATH) as _f:
    COST_EXT_HEADER = parse_header(_f.read())      # an eighth table (the #include of mpcrl.h is not followed)
COST_EXT_EXPORTS = list(COST_EXT_HEADER.functions)
COST_EXT_VERSION = COST_EXT_HEADER.constants["COST_EXT_VERSION"]
TRAJ_JVP_EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpcrl_traj_jvp_ext.h")   # the trajectory Jacobian-vector product, versioned on its own
if not os.path.exists(TRAJ_JVP_EXT_HEADER_PATH):
    raise ImportError(f"mpc4rl_amd: {TRAJ_JVP_EXT_HEADER_PATH} not found. The binding is read from the headers: keep include/ beside the package.")
with open(TRAJ_JVP_EXT_HEADER_PATH) as _f:
    TRAJ_JVP_EXT_HEADER = parse_header(_f.read())      # a ninth table (the #include of mpcrl_ext.h is not followed)
TRAJ_JVP_EXT_EXPORTS = list(TRAJ_JVP_EXT_HEADER.functions)
TRAJ_JVP_EXT_VERSION = TRAJ_JVP_EXT_HEADER.constants["TRAJ_JVP_EXT_VERSION"]
CHAIN_TRAJ_JVP_EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpcrl_chain_traj_jvp_ext.h")   # the trajectory JVP of the chain of masses, versioned on its own
if not os.path.exists(CHAIN_TRAJ_JVP_EXT_HEADER_PATH):
    raise ImportError(f"mpc4rl_amd: {CHAIN_TRAJ_JVP_EXT_HEADER_PATH} not found. The binding is read from the headers: keep include/ beside the package.")
with open(CHAIN_TRAJ_JVP_EXT_HEADER_PATH) as _f:
    CHAIN_TRAJ_JVP_EXT_HEADER = parse_header(_f.read())      # a tenth table (the #include of mpcrl_ext.h is not followed)
CHAIN_TRAJ_JVP_EXT_EXPORTS = list(CHAIN_TRAJ_JVP_EXT_HEADER.functions)
CHAIN_TRAJ_JVP_EXT_VERSION = CHAIN_TRAJ_JVP_EXT_HEADER.constants["CHAIN_TRAJ_JVP_EXT_VERSION"]
PROBE_EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpcrl_probe_ext.h")   # test probes of single kernel phases, versioned on their own
if not os.path.exists(PROBE_EXT_HEADER_PATH):
    raise ImportError(f"mpc4rl_amd: {PROBE_EXT_HEADER_PATH} not found. The binding is read from the headers: keep include/ beside the package.")
with open(PROBE_EXT_HEADER_PATH) as _f:
    PROBE_EXT_HEADER = parse_header(_f.read())      # a seventh table (the #include of mpcrl.h is not followed)
PROBE_EXT_EXPORTS = list(PROBE_EXT_HEADER.functions)
PROBE_EXT_VERSION = PROBE_EXT_HEADER.constants["PROBE_EXT_VERSION"]
PROBE_MX_SLOT, PROBE_MX_PIN, PROBE_MX_WANT_P = (PROBE_EXT_HEADER.constants[n] for n in ("PROBE_MX_SLOT", "PROBE_MX_PIN", "PROBE_MX_WANT_P"))
PROBE_CHAIN_EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpcrl_probe_chain_ext.h")   # the test probe of the vector sweeps' chains, versioned on its own
if not os.path.exists(PROBE_CHAIN_EXT_HEADER_PATH):
    raise ImportError(f"mpc4rl_amd: {PROBE_CHAIN_EXT_HEADER_PATH} not found. The binding is read from the headers: keep include/ beside the package.")
with open(PROBE_CHAIN_EXT_HEADER_PATH) as _f:
    PROBE_CHAIN_EXT_HEADER = parse_header(_f.read())      # a table of its own (the #include of mpcrl_probe_ext.h is not followed)
PROBE_CHAIN_EXT_EXPORTS = list(PROBE_CHAIN_EXT_HEADER.functions)
PROBE_CHAIN_EXT_VERSION = PROBE_CHAIN_EXT_HEADER.constants["PROBE_CHAIN_EXT_VERSION"]


def _constants(names: str):
    return tuple(HEADER.constants[n] for n in names.split())      # (KeyError: the header no longer has the name)


# the header's MPCRL_* #defines and enumerators under their Python names (the prefix dropped)
ABI_VERSION, NO_BOUND = _constants("ABI_VERSION NO_BOUND")
SENS_V, SENS_PI, RTI, COLD, COLD_DUAL, NO_BND_STORE, EXACT_QP = _constants("SENS_V SENS_PI RTI COLD COLD_DUAL NO_BND_STORE EXACT_QP")   # (EXACT_QP: test-only)
MODEL_CARTPOLE, MODEL_LINEAR, MODEL_CHAIN = _constants("MODEL_CARTPOLE MODEL_LINEAR MODEL_CHAIN")
COST_NLS, COST_EXTERNAL = _constants("COST_NLS COST_EXTERNAL")
BOUNDS_U0, BOUNDS_STAGE, BOUNDS_TERMINAL = _constants("BOUNDS_U0 BOUNDS_STAGE BOUNDS_TERMINAL")
E_ARG, E_MODEL, E_HIP, E_NOMEM = _constants("E_ARG E_MODEL E_HIP E_NOMEM")
_ERRORS = {v: "MPCRL_" + k for k, v in HEADER.constants.items() if k.startswith("E_")}

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class ProblemSpec(C.Structure):
    """MpcrlProblemSpec of include/mpcrl.h."""
    _fields_ = [
        ("model", C.c_int32), ("N", C.c_int32), ("nx", C.c_int32), ("nu", C.c_int32), ("np", C.c_int32),
        ("cost_kind", C.c_int32), ("dT", C.c_double), ("gamma", C.c_double), ("h", C.c_double), ("rk_steps", C.c_int32),
        ("tol", C.c_double), ("max_iter", C.c_int32),
        ("lb0", _dp), ("ub0", _dp), ("lb", _dp), ("ub", _dp), ("lbe", _dp), ("ube", _dp),
        ("soft", _ip), ("zl", _dp), ("zu", _dp), ("consts", _dp), ("n_consts", C.c_int32),
    ]


_FIELD = {"int32": C.c_int32, "double": C.c_double, "int32*": _ip, "double*": _dp}
if ProblemSpec._fields_ != [(n, _FIELD[k]) for n, k in HEADER.spec_fields]:
    raise ImportError(f"mpc4rl_amd: ProblemSpec no longer matches MpcrlProblemSpec of {HEADER_PATH}")

_CTYPE = {"int": C.c_int, "int64": C.c_int64, "double": C.c_double}      # a handle and every pointer: c_void_p
_lib = None
torch = None    # imported by load(): reading the header needs neither torch nor HIP
_plans = {}     # export -> (function, ((parameter, dtypes) ...) without the stream, takes a stream): what `call` needs, prepared by load()


def _ptr(t):
    """The device address of a tensor for a direct call of the library (tests, profiles/microbench); the package itself uses ``call``."""
    return None if t is None else C.c_void_p(t.data_ptr())


def load():
    """Returns the loaded library; raises RuntimeError (never falls back) when it is absent."""
    global _lib, torch
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"mpc4rl_amd: {LIB_PATH} not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    import torch
    lib = C.CDLL(LIB_PATH)
    lib.mpcrl_version.restype = C.c_int
    if lib.mpcrl_version() != ABI_VERSION and not os.environ.get("MPCRL_SKIP_ABI_CHECK"):   # (the override: A/B runs against older builds) extern "C" links whatever the signatures are: refuse a library built from another header
        raise RuntimeError(f"mpc4rl_amd: {LIB_PATH} reports ABI version {lib.mpcrl_version()}, this binding expects {ABI_VERSION}; rebuild it "
                           "(`python -c 'import __graft_entry__ as g; g.build()'`).")
    # what a tensor handed to a pointer parameter may hold: None = no tensor there, () = any (void *)
    dtypes = {"double*": (torch.float64,), "float*": (torch.float32,), "int32*": (torch.int32,), "int64*": (torch.int64,),
              "uint8*": (torch.uint8, torch.bool), "void*": ()}
    lib.mpcrl_ext_version.restype = C.c_int
    if lib.mpcrl_ext_version() != EXT_VERSION and not os.environ.get("MPCRL_SKIP_ABI_CHECK"):
        raise RuntimeError(f"mpc4rl_amd: {LIB_PATH} reports extension version {lib.mpcrl_ext_version()}, this binding expects {EXT_VERSION}; "
                           "rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`).")
    lib.mpcrl_chain_ext_version.restype = C.c_int
    if lib.mpcrl_chain_ext_version() != CHAIN_EXT_VERSION and not os.environ.get("MPCRL_SKIP_ABI_CHECK"):
        raise RuntimeError(f"mpc4rl_amd: {LIB_PATH} reports chain extension version {lib.mpcrl_chain_ext_version()}, this binding expects "
                           f"{CHAIN_EXT_VERSION}; rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`).")
    lib.mpcrl_traj_ext_version.restype = C.c_int
    if lib.mpcrl_traj_ext_version() != TRAJ_EXT_VERSION and not os.environ.get("MPCRL_SKIP_ABI_CHECK"):
        raise RuntimeError(f"mpc4rl_amd: {LIB_PATH} reports trajectory extension version {lib.mpcrl_traj_ext_version()}, this binding expects "
                           f"{TRAJ_EXT_VERSION}; rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`).")
    lib.mpcrl_chain_traj_ext_version.restype = C.c_int
    if lib.mpcrl_chain_traj_ext_version() != CHAIN_TRAJ_EXT_VERSION and not os.environ.get("MPCRL_SKIP_ABI_CHECK"):
        raise RuntimeError(f"mpc4rl_amd: {LIB_PATH} reports chain trajectory extension version {lib.mpcrl_chain_traj_ext_version()}, this "
                           f"binding expects {CHAIN_TRAJ_EXT_VERSION}; rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`).")
    older = bool(os.environ.get("MPCRL_SKIP_ABI_CHECK"))      # an A/B run against an older build: what it lacks is left unbound
    if not (older and not hasattr(lib, "mpcrl_bound_ext_version")):
        lib.mpcrl_bound_ext_version.restype = C.c_int
    if not older and lib.mpcrl_bound_ext_version() != BOUND_EXT_VERSION:
        raise RuntimeError(f"mpc4rl_amd: {LIB_PATH} reports bound extension version {lib.mpcrl_bound_ext_version()}, this binding expects "
                           f"{BOUND_EXT_VERSION}; rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`).")
    if not (older and not hasattr(lib, "mpcrl_cost_ext_version")):
        lib.mpcrl_cost_ext_version.restype = C.c_int
    if not older and lib.mpcrl_cost_ext_version() != COST_EXT_VERSION:
        raise RuntimeError(f"mpc4rl_amd: {LIB_PATH} reports cost extension version {lib.mpcrl_cost_ext_version()}, this binding expects "
                           f"{COST_EXT_VERSION}; rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`).")
    if not (older and not hasattr(lib, "mpcrl_traj_jvp_ext_version")):
        lib.mpcrl_traj_jvp_ext_version.restype = C.c_int
    if not older and lib.mpcrl_traj_jvp_ext_version() != TRAJ_JVP_EXT_VERSION:
        raise RuntimeError(f"mpc4rl_amd: {LIB_PATH} reports trajectory JVP extension version {lib.mpcrl_traj_jvp_ext_version()}, this binding "
                           f"expects {TRAJ_JVP_EXT_VERSION}; rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`).")
    if not (older and not hasattr(lib, "mpcrl_chain_traj_jvp_ext_version")):
        lib.mpcrl_chain_traj_jvp_ext_version.restype = C.c_int
    if not older and lib.mpcrl_chain_traj_jvp_ext_version() != CHAIN_TRAJ_JVP_EXT_VERSION:
        raise RuntimeError(f"mpc4rl_amd: {LIB_PATH} reports chain trajectory JVP extension version {lib.mpcrl_chain_traj_jvp_ext_version()}, "
                           f"this binding expects {CHAIN_TRAJ_JVP_EXT_VERSION}; rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`).")
    if not (older and not hasattr(lib, "mpcrl_probe_ext_version")):
        lib.mpcrl_probe_ext_version.restype = C.c_int
        if not older and lib.mpcrl_probe_ext_version() != PROBE_EXT_VERSION:
            raise RuntimeError(f"mpc4rl_amd: {LIB_PATH} reports probe extension version {lib.mpcrl_probe_ext_version()}, this binding expects "
                               f"{PROBE_EXT_VERSION}; rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`).")
    if not (older and not hasattr(lib, "mpcrl_probe_chain_ext_version")):
        lib.mpcrl_probe_chain_ext_version.restype = C.c_int
        if not older and lib.mpcrl_probe_chain_ext_version() != PROBE_CHAIN_EXT_VERSION:
            raise RuntimeError(f"mpc4rl_amd: {LIB_PATH} reports chain probe extension version {lib.mpcrl_probe_chain_ext_version()}, this binding "
                               f"expects {PROBE_CHAIN_EXT_VERSION}; rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`).")
    for name, (ret, params) in (list(HEADER.functions.items()) + list(EXT_HEADER.functions.items()) + list(CHAIN_EXT_HEADER.functions.items())
                                + list(TRAJ_EXT_HEADER.functions.items()) + list(CHAIN_TRAJ_EXT_HEADER.functions.items())
                                + list(BOUND_EXT_HEADER.functions.items()) + list(COST_EXT_HEADER.functions.items())
                                + list(TRAJ_JVP_EXT_HEADER.functions.items()) + list(CHAIN_TRAJ_JVP_EXT_HEADER.functions.items())
                                + list(PROBE_EXT_HEADER.functions.items()) + list(PROBE_CHAIN_EXT_HEADER.functions.items())):
        if older and (name in BOUND_EXT_HEADER.functions or name in COST_EXT_HEADER.functions or name in TRAJ_JVP_EXT_HEADER.functions
                      or name in CHAIN_TRAJ_JVP_EXT_HEADER.functions or name in PROBE_EXT_HEADER.functions
                      or name in PROBE_CHAIN_EXT_HEADER.functions) and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = _CTYPE[ret]
        fn.argtypes = [_CTYPE.get(kind, C.c_void_p) for _, kind in params]
        stream = bool(params) and params[-1] == ("stream", "void*")
        _plans[name] = (fn, tuple((p, dtypes.get(kind)) for p, kind in (params[:-1] if stream else params)), stream)
    _lib = lib
    return lib


def call(name: str, *args, device=None) -> int:
    """Calls the export ``name`` with ``args`` checked against its prototype in the header, and returns what it returns (>= 0); a
    negative return raises RuntimeError.  A trailing ``void *stream`` is not given: ``call`` passes the current stream of ``device``
    (required then; inside a capture that is the capture stream) and runs under ``torch.cuda.device(device)``.  A tensor stands for its
    device address and must be handed to a pointer parameter of its dtype and live on ``device`` (strides are the caller's contract);
    None is NULL; anything else (ints, floats, ctypes arrays, byref) goes to ctypes as it is.  A refused argument raises TypeError or
    ValueError before anything is called."""
    if _lib is None:
        load()
    fn, params, stream = _plans[name]
    if len(args) != len(params):
        raise TypeError(f"{name} takes {len(params)} arguments ({', '.join(p for p, _ in params)}{' and the stream' if stream else ''}), "
                        f"{len(args)} were given")
    if stream and device is None:
        raise TypeError(f"{name} launches on a stream: `device` is required")
    index = None
    if device is not None:
        index = device.index if isinstance(device, torch.device) else torch.device(device).index
        if index is None:       # "cuda": the current device
            index = torch.cuda.current_device()
    argv = []
    for a, (pname, dtypes) in zip(args, params):
        if isinstance(a, torch.Tensor):
            if dtypes is None:
                raise TypeError(f"{name}: parameter {pname} takes no array, a tensor was given")
            if dtypes and a.dtype not in dtypes:
                raise TypeError(f"{name}: parameter {pname} points to {dtypes[0]}, the tensor given holds {a.dtype}")
            if not a.is_cuda or a.device.index != index:
                raise ValueError(f"{name}: the tensor given for {pname} lives on {a.device}, the call is for "
                                 f"{'no device' if index is None else f'cuda:{index}'}")
            a = a.data_ptr()
        argv.append(a)
    if stream:
        with torch.cuda.device(index):
            rc = fn(*argv, torch.cuda.current_stream(index).cuda_stream)
    else:
        rc = fn(*argv)
    if rc < 0:
        raise RuntimeError(f"{name} failed with {rc}" + (f" ({_ERRORS[rc]})" if rc in _ERRORS else ""))
    return rc


def workspace(name: str, *dims, device):
    """A zeroed uint8 tensor on ``device`` of the size the export ``name`` (a ``*_workspace_bytes``) returns for ``dims``."""
    nbytes = call(name, *dims)      # first: the call is what loads the library (and torch) on a first use
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)
