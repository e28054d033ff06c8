"""mpcrl_debug_mx_chain of include/mpcrl_probe_chain_ext.h without a GPU: the export is declared in a header and a table of the binding
of its own and nowhere else (the table of include/mpcrl_probe_ext.h is what it was), defined in the probe's translation unit with the
copy of the earlier chain it is compared against, present in the built library with the header's version, and every argument the probe
cannot run is refused before anything touches a device (the refusals are host code: the arrays here are host memory that a refused
call never reads)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc4rl_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from mpc4rl_amd import _lib
    return _lib.load()


def test_chain_probe_is_declared_in_a_header_of_its_own():
    from mpc4rl_amd import _lib
    assert _lib.PROBE_CHAIN_EXT_EXPORTS == ["mpcrl_probe_chain_ext_version", "mpcrl_debug_mx_chain"]
    assert os.path.basename(_lib.PROBE_CHAIN_EXT_HEADER_PATH) == "mpcrl_probe_chain_ext.h" and not _lib.PROBE_CHAIN_EXT_HEADER.spec_fields
    ret, params = _lib.PROBE_CHAIN_EXT_HEADER.functions["mpcrl_debug_mx_chain"]
    assert ret == "int" and params == [("slots_in", "double*"), ("N", "int"), ("forward", "int"), ("which", "int"), ("slots_out", "double*"),
                                       ("stream", "void*")]
    others = (_lib.HEADER, _lib.EXT_HEADER, _lib.CHAIN_EXT_HEADER, _lib.TRAJ_EXT_HEADER, _lib.CHAIN_TRAJ_EXT_HEADER, _lib.BOUND_EXT_HEADER,
              _lib.COST_EXT_HEADER, _lib.TRAJ_JVP_EXT_HEADER, _lib.CHAIN_TRAJ_JVP_EXT_HEADER, _lib.PROBE_EXT_HEADER)
    for other in others:
        assert not set(_lib.PROBE_CHAIN_EXT_EXPORTS) & set(other.functions)
    assert _lib.PROBE_EXT_EXPORTS == ["mpcrl_probe_ext_version", "mpcrl_debug_mx_factor"] and _lib.PROBE_EXT_VERSION == 1
    # the slot constant is the factor probe's: the new header includes that header and defines none of its own
    assert "PROBE_MX_SLOT" not in _lib.PROBE_CHAIN_EXT_HEADER.constants
    text = open(_lib.PROBE_CHAIN_EXT_HEADER_PATH).read()
    assert '#include "mpcrl_probe_ext.h"' in text


def test_version_is_the_headers(lib):
    from mpc4rl_amd import _lib
    assert _lib.PROBE_CHAIN_EXT_VERSION == _lib.PROBE_CHAIN_EXT_HEADER.constants["PROBE_CHAIN_EXT_VERSION"] == 1
    assert lib.mpcrl_probe_chain_ext_version() == _lib.PROBE_CHAIN_EXT_VERSION
    assert lib.mpcrl_probe_ext_version() == _lib.PROBE_EXT_VERSION


def test_probe_unit_defines_the_chain_probe_and_its_reference_copy(lib):
    unit = open(os.path.join(CSRC, "mpcrl_probe.hip")).read()
    for name in ("mpcrl_debug_mx_chain", "mpcrl_probe_chain_ext_version"):
        assert re.search(r"^int " + name + r"\(", unit, flags=re.M), name
    assert "struct MxChainBefore" in unit and unit.count("void mx_chain()") == 1       # the earlier form: in this unit, once
    kernel = open(os.path.join(CSRC, "small_kernel.hpp")).read()
    assert kernel.count("void mx_chain()") == 1 and "MxChainBefore" not in kernel      # the shipped form: the kernels' own
    assert hasattr(lib, "mpcrl_debug_mx_chain")


def test_chain_probe_refuses_what_it_cannot_run(lib):
    from mpc4rl_amd import _lib
    buf = (ctypes.c_double * (64 * _lib.PROBE_MX_SLOT))()
    fn = lib.mpcrl_debug_mx_chain
    for N, forward, which in ((0, 1, 1), (-1, 1, 1), (64, 0, 1), (20, 2, 1), (20, -1, 0), (20, 1, 2), (20, 0, -1)):
        assert fn(buf, N, forward, which, buf, None) == _lib.E_ARG, (N, forward, which)
    assert fn(None, 20, 1, 1, buf, None) == _lib.E_ARG
    assert fn(buf, 20, 1, 1, None, None) == _lib.E_ARG
