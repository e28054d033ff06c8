"""include/mpcrl_probe_ext.h and its table in the binding (no GPU): the probe exports are declared there and nowhere else, defined in
their own translation unit, and the constants the header states are those of the kernels' slot layout."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_probe_header_is_a_table_of_its_own():
    from mpc4rl_amd import _lib
    assert _lib.PROBE_EXT_EXPORTS == ["mpcrl_probe_ext_version", "mpcrl_debug_mx_factor"]
    assert _lib.PROBE_EXT_HEADER.constants["PROBE_EXT_VERSION"] == _lib.PROBE_EXT_VERSION == 1
    assert os.path.basename(_lib.PROBE_EXT_HEADER_PATH) == "mpcrl_probe_ext.h" and not _lib.PROBE_EXT_HEADER.spec_fields
    ret, params = _lib.PROBE_EXT_HEADER.functions["mpcrl_debug_mx_factor"]
    assert ret == "int" and params == [("slots_in", "double*"), ("N", "int"), ("flags", "int"), ("which", "int"), ("slots_out", "double*"),
                                       ("ok_out", "double*"), ("stream", "void*")]
    others = (_lib.HEADER, _lib.EXT_HEADER, _lib.CHAIN_EXT_HEADER, _lib.TRAJ_EXT_HEADER, _lib.CHAIN_TRAJ_EXT_HEADER, _lib.BOUND_EXT_HEADER)
    for other in others:
        assert not set(_lib.PROBE_EXT_EXPORTS) & set(other.functions)


def test_probe_unit_defines_what_the_header_declares():
    from mpc4rl_amd import _lib
    csrc = os.path.join(ROOT, "mpc4rl_amd", "csrc")
    unit = open(os.path.join(csrc, "mpcrl_probe.hip")).read()
    for name in _lib.PROBE_EXT_EXPORTS:
        assert re.search(r"^int " + name + r"\(", unit, flags=re.M), name
    assert "probe.o" in open(os.path.join(csrc, "Makefile")).read()
    kernel = open(os.path.join(csrc, "small_kernel.hpp")).read()
    assert re.search(r"MSLOT = %d\b" % _lib.PROBE_MX_SLOT, kernel)
    assert (_lib.PROBE_MX_PIN, _lib.PROBE_MX_WANT_P) == (1, 2)
