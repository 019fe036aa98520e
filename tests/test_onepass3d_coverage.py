"""Every instance of the one-pass 3-D level kernels in the shipped library is reached by a row of the oracle-checked case table
(CPU only: the .so is unbundled and disassembled with tools/isa_check.py's helpers).

k_fwd3d_one<T, RPL, F, NW> and k_inv3d_one<T, RPL, F, NW> are picked per level from the line length (tests/onepass3d_cases.py
restates the launchers' choice).  A template instance added to a launcher without a row in that table fails here, before a GPU
ever runs it unchecked.
"""
import os
import re
import sys
import tempfile

import pytest

import onepass3d_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wavelets.jl_amd", "libwavelets_mi355x.so")

# Itanium mangling of wl::k_fwd3d_one<float, 2, 10, 4>(...): _ZN2wl11k_fwd3d_oneIfLi2ELi10ELi4EEEv...
_re_sym = re.compile(r"_ZN2wl11k_(fwd3d|inv3d)_oneI([fd])Li(\d+)ELi(\d+)ELi(\d+)EEEv")
_TYPES = {"f": "float", "d": "double"}


def _isa():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import isa_check
    return isa_check


@pytest.fixture(scope="module")
def instances():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    m = _isa()
    found = {"fwd3d": set(), "inv3d": set()}
    with tempfile.TemporaryDirectory(prefix="wl_3d1_") as tmp:
        for co in m.extract_code_objects(LIB, tmp):
            with open(co, "rb") as f:
                if b"_oneI" not in f.read():
                    continue                # (the translation units without these kernels: not worth a disassembly)
            for name in m.parse_functions(m.disassemble(co)):
                g = _re_sym.match(name)
                if g:
                    found[g.group(1)].add((_TYPES[g.group(2)], int(g.group(3)), int(g.group(4)), int(g.group(5))))
    return found


def test_library_holds_the_launchers_instances(instances):
    """the symbols match what the launchers can pick (the names did not drift, nothing was dropped)"""
    fwd = {("float", r, F, w) for F in (2, 4, 6, 8) for r, ws in ((2, (1, 2, 4, 8)), (4, (1, 2, 4))) for w in ws}
    fwd |= {("float", 2, 10, w) for w in (1, 2, 4, 8)}
    fwd |= {("double", 2, F, w) for F in (2, 4, 6, 8) for w in (1, 2, 4, 8)}
    inv = {("float", r, F, w) for F in (2, 4, 6, 8) for r, ws in ((2, (1, 2, 4, 8)), (4, (1, 2, 4))) for w in ws}
    inv |= {("double", 2, F, w) for F in (2, 4, 6, 8) for w in (1, 2, 4)}
    assert instances["fwd3d"] >= fwd, sorted(fwd - instances["fwd3d"])
    assert instances["inv3d"] >= inv, sorted(inv - instances["inv3d"])


def test_every_forward_instance_has_an_oracle_checked_row(instances):
    reached = C.fwd_cases_by_instance()
    missing = sorted(instances["fwd3d"] - set(reached))
    assert not missing, "k_fwd3d_one instances without a row in tests/onepass3d_cases.py FWD_CASES: %s" % missing
    # the table reaches nothing the library lacks (a stale restatement of the launcher)
    assert set(reached) <= instances["fwd3d"], sorted(set(reached) - instances["fwd3d"])


def test_every_inverse_instance_has_an_oracle_checked_row(instances):
    reached = C.inv_cases_by_instance()
    missing = sorted(instances["inv3d"] - set(reached))
    assert not missing, "k_inv3d_one instances without a row in tests/onepass3d_cases.py INV_CASES: %s" % missing
    assert set(reached) <= instances["inv3d"], sorted(set(reached) - instances["inv3d"])


def test_ten_tap_multi_wave_instances_march_more_than_one_group():
    """10 taps: steps come in groups of U = 5 and the LDS exchange has one barrier per step, so consecutive steps must not share an
    exchange buffer.  A wrong choice shows only on lines of more than one wave (a wave can run a step ahead) and across a group
    boundary (segments of >= 20 columns) -- every such instance has rows of that kind, on lines that fill their waves and lines
    that do not"""
    reached = C.fwd_cases_by_instance()
    for nw in (2, 4, 8):
        rows = [(shape, TJ) for shape, L, f, TJ in reached.get(("float", 2, 10, nw), ()) if TJ // 2 > 5]
        assert rows, ("float", 2, 10, nw)
    for n0 in (256, 512, 1024):
        assert any(s[0] == n0 and C.fwd_segment(s[1], 10, 64) >= 20 for s, L in C.FWD_CASES), n0
    assert any(s[0] % 128 and C.fwd_instance("float", 10, s[0])[3] > 1 and C.fwd_segment(s[1], 10, 64) >= 20 for s, L in C.FWD_CASES)


def test_restated_segment_length():
    """fwd_segment against launch_fwd3d_f by hand: the largest multiple of the ring <= the request and the extent, a divisor of
    n1 within two rings below it preferred"""
    assert C.fwd_segment(16, 10, 64) == 10
    assert C.fwd_segment(64, 10, 64) == 60
    assert C.fwd_segment(48, 10, 64) == 40
    assert C.fwd_segment(40, 10, 64) == 40
    assert C.fwd_segment(32, 10, 64) == 30
    assert C.fwd_segment(64, 8, 64) == 64
    assert C.fwd_segment(70, 8, 64) == 64
    assert C.fwd_segment(48, 8, 64) == 48
    assert C.fwd_segment(16, 8, 8) == 8
