"""Every kernel instance in the shipped library is launched by a row of the oracle-checked instance table, or is shown to be
unreachable (CPU only: the symbols of the built library against the record of a kernel trace).

tests/instances_reached.json is what tools/instance_trace.py read from a rocprofv3 kernel trace of every row of
tests/instance_cases.py (family -> template argument strings).  The library's kernel symbols are listed and normalised by the same
tool.  A template instance added to a launcher without a row and a fresh trace fails here, before a GPU runs it unchecked -- the
promise test_onepass3d_coverage.py makes for its two kernels, for all of them.

EXEMPT (instance_cases.py) admits one reason: no argument and no option selects the instance, with the launcher line that shows it.
"""
import json
import os
import sys

import pytest

import instance_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wavelets.jl_amd", "libwavelets_mi355x.so")
REACHED = os.path.join(ROOT, "tests", "instances_reached.json")


def _flat(d):
    return {(f, a) for f, s in d.items() for a in s}


@pytest.fixture(scope="module")
def shipped():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import instance_trace
    return instance_trace.shipped(LIB)


@pytest.fixture(scope="module")
def reached():
    with open(REACHED) as f:
        return {fam: set(args) for fam, args in json.load(f).items()}


def test_normalise_gives_one_name_per_instance():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    from instance_trace import normalise
    want = ("k_inv2d_lds_long", "float, 10, 1, 2, 0, 2")
    assert normalise("void wl::k_inv2d_lds_long<float, 10, 1, 2, 0, 2>(wl::InvLongArgs<float, 10>)") == want
    assert normalise("void wl::(anonymous namespace)::k_inv2d_lds_long<float, (int)10, 1, 2u, false, 2l>(wl::InvLongArgs<float, 10>)") == want
    assert normalise("void wl::(anonymous namespace)::k_bb_up(double const*, long)") == ("k_bb_up", "")
    assert normalise("void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>, std::array<char*, 1ul> >(int)") is None


def test_shipped_is_reached_or_exempt(shipped, reached):
    ship, reach = _flat(shipped), _flat(reached)
    stale = sorted(reach - ship)
    assert not stale, "the trace names instances the library does not ship (a stale record): %s" % stale
    missing = sorted(ship - reach - set(IC.EXEMPT))
    assert not missing, "shipped instances with no row in tests/instance_cases.py and no fresh trace: %s" % missing


def test_exemptions_exist_and_are_unreached(shipped, reached):
    ship, reach = _flat(shipped), _flat(reached)
    gone = sorted(set(IC.EXEMPT) - ship)
    assert not gone, "exempt instances that the library no longer ships: %s" % gone
    hit = sorted(set(IC.EXEMPT) & reach)
    assert not hit, "exempt instances that the trace reached: %s" % hit
    for key, reason in IC.EXEMPT.items():
        assert ".hip:" in reason or ".h:" in reason, (key, "an exemption cites the launcher line that shows the instance unreachable")


def test_every_larger_family_is_reached(shipped, reached):
    none = sorted(f for f, s in shipped.items() if len(s) > 2 and not (reached.get(f, set()) & s))
    assert not none, none


def test_the_one_pass_3d_account_agrees(reached):
    for fam, args in IC.ONEPASS3D.items():
        missing = sorted(args - reached.get(fam, set()))
        assert not missing, "%s instances that onepass3d_cases.py reaches and the trace did not see: %s" % (fam, missing)
