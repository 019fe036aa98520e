"""The user-defined lifting scheme table (tests/lifting_schemes.py) on the CPU: its restatement of the known shapes matches
wl_lift_shapes.h / match_shape, every shape has a twin, the twins / custom shapes / near misses are what they claim to be, the
transforms stay far from overflow, and two checks that do not rely on the oracle's lifting loops (a hand-computed answer and
the Float64 round trip)."""
import os
import re

import numpy as np
import pytest

import lifting_schemes as LS
from conftest import rng_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wavelets.jl_amd", "csrc")

_re_shape = re.compile(r"template\s*<>\s*struct\s+Shape<(\d+)>\s*\{\s*static\s+constexpr\s+int\s+NS\s*=\s*(\d+);\s*"
                       r"static\s+constexpr\s+StepShape\s+S\[\d+\]\s*=\s*\{(.*?)\};\s*\};", re.S)
_re_step = re.compile(r"\{\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*\}")


def parse_shapes(text):
    out = {}
    for m in _re_shape.finditer(text):
        steps = tuple(tuple(int(v) for v in s) for s in _re_step.findall(m.group(3)))
        assert len(steps) == int(m.group(2)), m.group(0)
        out[int(m.group(1))] = steps
    return out


def header_shapes():
    with open(os.path.join(CSRC, "wl_lift_shapes.h")) as f:
        text = f.read()
    n_spec = len(re.findall(r"struct\s+Shape<\d+>\s*\{", text))
    shapes = parse_shapes(text)
    assert len(shapes) == n_spec, "a Shape<ID> specialisation the parser does not understand"
    return shapes


def test_parser_sees_an_added_shape():
    """the restatement check below would notice a new specialisation (a Shape<6> added to the header)"""
    with open(os.path.join(CSRC, "wl_lift_shapes.h")) as f:
        text = f.read()
    extra = text.replace("// dependency cone", "template <> struct Shape<6> { static constexpr int NS = 1; static constexpr StepShape "
                         "S[1] = {{0, 3, 2}}; };\n// dependency cone", 1)
    assert parse_shapes(extra)[6] == ((0, 3, 2),)
    assert parse_shapes(extra) != LS.SHAPES


def test_shape_restatement_matches_the_header():
    """shape_id restates match_shape: the same shapes, in the order match_shape tries them (ids 0 .. 5 in turn, each through
    by_shape, whose cases are the ids the header has a Shape<ID> for)"""
    assert header_shapes() == LS.SHAPES
    with open(os.path.join(CSRC, "wl_lift_shapes.h")) as f:
        src = f.read()
    body = re.search(r"inline int match_shape\(const LiftScheme<T> &sc\)\s*\{(.*?)\n\}", src, re.S).group(1)
    lo, hi = re.search(r"for \(int id = (\d+); id <= (\d+); \+\+id\)", body).groups()
    assert "by_shape(id, false," in body and "return id;" in body
    dispatch = re.search(r"inline R by_shape\(int id, R none, F f\)\s*\{(.*?)\n\}", src, re.S).group(1)
    cases = re.findall(r"case (\d+): return f\(ShapeId<(\d+)>\(\)\);", dispatch)
    assert all(a == b for a, b in cases) and dispatch.count("case ") == len(cases)
    tried = [int(a) for a, _ in cases if int(lo) <= int(a) <= int(hi)]
    assert tried == sorted(LS.SHAPES) == list(range(int(lo), int(hi) + 1)), tried


def test_every_shape_has_a_twin(W):
    """the forward twin of a shape hits its even ID, the inverse (make_scheme reverses the steps) the odd one after it"""
    reached = {}
    for name in LS.TWINS:
        sch = LS.scheme(W, name)
        fw, inv = LS.shape_id(sch), LS.shape_id(sch, fw=False)
        assert fw >= 0 and fw % 2 == 0 and inv == fw + 1, (name, fw, inv)
        reached[fw] = reached[inv] = name
    assert sorted(reached) == sorted(header_shapes()), "shapes without a twin in tests/lifting_schemes.py: %s" % (
        sorted(set(header_shapes()) - set(reached)))


def test_reversed_twins_have_the_shape_of_the_other_direction(W):
    """a reversed twin's forward steps have an inverse shape (odd ID), its inverse the forward shape before it"""
    assert sorted(LS.REVERSED_TWINS) == sorted("rev_" + n for n in LS.TWINS)
    for name in LS.REVERSED_TWINS:
        sch, tw = LS.scheme(W, name), LS.scheme(W, name[4:])
        assert LS.steps_of(sch) == LS.steps_of(tw)[::-1] and (sch.norm1, sch.norm2) == (tw.norm1, tw.norm2), name
        assert LS.shape_id(sch) in (1, 3, 5) and LS.shape_id(sch, fw=False) == LS.shape_id(sch) - 1, name
        assert LS.shape_id(sch) == LS.shape_id(tw, fw=False), name


def _ref_coefs(W):
    out = set()
    for nm in LS.REFERENCE:
        sch = W.wavelet(getattr(W.WT, nm), W.WT.Lifting)
        for st in sch.step:
            out.update(float(c) for c in st.param.coef)
    return out


def test_twins_differ_from_their_table_scheme_in_every_coefficient(W):
    ref_c = _ref_coefs(W)
    for name, ref in LS.TWIN_OF.items():
        tw, rs = LS.scheme(W, name), W.wavelet(getattr(W.WT, ref), W.WT.Lifting)
        assert LS.steps_of(tw) == LS.steps_of(rs), name
        for st in tw.step:
            c = [float(v) for v in st.param.coef]
            assert not set(c) & ref_c, (name, c)
            if len(c) == 2:
                assert c[0] != c[1] and c[0] != -c[1], (name, c)
        norms = {float(v) for s in LS.REFERENCE for v in (W.wavelet(getattr(W.WT, s), W.WT.Lifting).norm1,
                                                            W.wavelet(getattr(W.WT, s), W.WT.Lifting).norm2)}
        assert tw.norm1 != tw.norm2 and not {tw.norm1, tw.norm2} & norms, name


def test_custom_shapes_and_near_misses_match_no_known_shape(W):
    for name in list(LS.CUSTOM) + list(LS.NEAR_MISSES) + list(LS.LARGE_SHIFTS):
        sch = LS.scheme(W, name)
        assert LS.shape_id(sch) == -1 and LS.shape_id(sch, fw=False) == -1, name
        iu, nc, sh, cf = sch.flatten()
        assert len(iu) <= 16 and all(1 <= v <= 3 for v in nc), name
    steps = {name: LS.steps_of(LS.scheme(W, name)) for name in LS.CUSTOM}
    assert any(nc == 3 for s in steps.values() for _, nc, _ in s)
    shifts = {sh for s in steps.values() for _, _, sh in s}
    assert {2, -2, 3, -3, 5, -5} <= shifts and max(abs(v) for v in shifts) > 4096
    assert {len(s) for s in steps.values()} >= {0, 1, 5, 16}
    # every near miss is exactly one field (type, nc, shift) or one step away from its table scheme
    for name in LS.NEAR_MISSES:
        ref = name.split("_")[1]
        a, b = LS.steps_of(LS.scheme(W, name)), LS.steps_of(W.wavelet(getattr(W.WT, ref), W.WT.Lifting))
        if len(a) == len(b):
            diff = [(x, y) for s, t in zip(a, b) for x, y in zip(s, t) if x != y]
            assert len(diff) == 1, (name, diff)
        else:
            assert abs(len(a) - len(b)) == 1 and (a[:len(b)] == b or b[:len(a)] == a), name


def test_large_shifts_reach_the_int32_limits(W):
    sh = {s for name in LS.LARGE_SHIFTS for _, _, s in LS.steps_of(LS.scheme(W, name))}
    assert {2 ** 20 + 3, -(2 ** 20 + 3), 2 ** 31 - 1, -(2 ** 31 - 1), -2 ** 31} <= sh


def test_shift_outside_int32_is_refused_by_flatten(W):
    for v in (2 ** 31, -2 ** 31 - 1):
        sch = W.GLS(([W.WT.make_lsstep(W.WT.Update, [0.5], v)], 1.0, 1.0, "x"))
        with pytest.raises(OverflowError):
            sch.flatten()


# inputs of the GPU tests' largest transforms (test_gpu_lifting_schemes.py and the twins' rows of the lifting tests)
GROWTH_SHAPES = ((1 << 18,), (32768,), (8192,), (2048,), (1024, 1024), (128, 128), (64, 64, 64), (16, 16, 16), (12,), (2,))


def test_growth_stays_far_from_overflow(oracle, W):
    """full-depth Float64 transforms of the test inputs: max |y| < 1e30 for every scheme of the table (Float32 then has
    eight decades of headroom)"""
    for shape in GROWTH_SHAPES:
        x = rng_array(shape, np.float64, 3 + len(shape))
        L = W.maxtransformlevels(x)
        for name in LS.ALL:
            y = oracle.dwt_lifting(x, LS.scheme(W, name), L)
            assert np.isfinite(y).all() and np.abs(y).max() < 1e30, (name, shape, np.abs(y).max())


def test_known_answer_one_predict_step(oracle, W):
    """by hand: one Predict step with coefficients (a, b), shift 1, norms (n1, n2), on a delta at sample 2k+1 of a line of 8.
    After the split s = x[0::2] = 0 and d = x[1::2] = e_k.  Forward coefficients are negated (makescheme), so
    s[j] = -(a d[j-1] + b d[j]) (indices mod 4); then s *= n1, d *= n2."""
    a, b, n1, n2 = 0.375, -1.25, 1.5, 0.75
    sch = W.GLS(([W.WT.make_lsstep(W.WT.Predict, [a, b], 1)], n1, n2, "kat"))
    for k in range(4):
        x = np.zeros(8)
        x[2 * k + 1] = 1.0
        s = np.zeros(4)
        s[(k + 1) % 4] += -a * n1
        s[k] += -b * n1
        d = np.zeros(4)
        d[k] = n2
        assert np.array_equal(oracle.dwt_lifting(x, sch, 1), np.concatenate([s, d])), k
    # a delta in the s half is untouched by a Predict step
    x = np.zeros(8)
    x[4] = 1.0
    assert np.array_equal(oracle.dwt_lifting(x, sch, 1), np.array([0, 0, n1, 0, 0, 0, 0, 0.0]))


def test_float64_round_trip_every_table_scheme(oracle, W):
    """idwt(dwt(x)) == x within 1e-10 relative (Float64: the steps are exactly invertible and only rounding remains, amplified by
    the growth of the near misses -- up to ~1e-11 measured; a wrong step order or sign is off by O(1))"""
    for shape in ((1024,), (12,), (2,), (64, 64), (8, 8, 8)):
        x = rng_array(shape, np.float64, sum(shape))
        L = W.maxtransformlevels(x)
        for name in list(LS.ALL) + list(LS.REFERENCE):
            sch = LS.scheme(W, name)
            xr = oracle.dwt_lifting(oracle.dwt_lifting(x, sch, L), sch, L, fw=False)
            assert np.linalg.norm(xr - x) <= 1e-10 * np.linalg.norm(x), (name, shape, np.linalg.norm(xr - x) / np.linalg.norm(x))
