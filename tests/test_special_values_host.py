"""The special-value cases of tests/special_values_cases.py, as far as a CPU can check them: every (recipe, class) pair has in the
oracle's output what the class is there for; the recipes cover every kernel name the transform entry points can report; the
comparison itself rejects what it must; and every kernel descriptor of the two shipped libraries keeps Float32 and Float64 / Float16
denormals (read from the descriptors alone: .amdhsa_float_denorm_mode_32 / _16_64 = 3)."""
import glob
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import special_values_cases as SV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wavelets.jl_amd", "csrc")
LIBS = [os.path.join(ROOT, "wavelets.jl_amd", n) for n in ("libwavelets_mi355x.so", "libwavelets_mi355x_fma.so")]
_re_name = re.compile(r'"(k_[A-Za-z0-9_+]+)"')        # (composite tier names, "k_a+k_b", and capitals included)


# ---- the classes are not vacuous -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rd", SV.recipe_cases(), ids=SV.case_id)
def test_every_pair_meets_its_class_condition(W, oracle, rd):
    r, dtype = rd
    bad = []
    for wname in r.wavelets:
        for cls in SV.CLASSES:
            if (r.name, cls) in SV.SKIPS:
                continue
            x, fwd, inv_in, inv, dir_in, dir_out = SV.reference(oracle, W, r, dtype, wname, cls)
            assert cls in ("nan_corner", "nan_last", "inf_pair") or np.isfinite(x).all()
            if cls in ("nan_corner", "nan_last"):                  # (their condition is stated at L = 1)
                fwd, inv = SV.reference_one_level(oracle, W, r, dtype, wname, cls)
            assert dir_in is None or cls == "inf_pair" or np.isfinite(dir_in).all()
            for tag, out in (("fwd", fwd), ("inv", inv), ("inv_direct", dir_out)):
                if out is None:
                    continue
                miss = SV.condition(cls, out, tag == "fwd" and not SV.ENTRIES[r.entry].synthesis, wname == "haar", tag == "inv_direct")
                if miss is not None:
                    bad.append((wname, cls, tag, miss))
    assert not bad, bad


def test_skips_are_few_and_real(W, oracle):
    names = {r.name for r in SV.RECIPES}
    assert all(n in names and c in SV.CLASSES and reason for (n, c), reason in SV.SKIPS.items()), SV.SKIPS
    per = {}
    for (n, c) in SV.SKIPS:
        per.setdefault(n, set()).add(c)
    assert all(len(v) == 1 for v in per.values()), per                      # at most one class per recipe
    pairs = len(SV.RECIPES) * len(SV.CLASSES)
    assert len(SV.SKIPS) <= 0.10 * pairs, (len(SV.SKIPS), pairs)
    # a skipped pair does miss its condition for some wavelet and element type (a stale entry fails here)
    for (n, c) in SV.SKIPS:
        r = next(q for q in SV.RECIPES if q.name == n)
        missed = False
        for dtype in r.dtypes:
            for wname in r.wavelets:
                x, fwd, inv_in, inv, dir_in, dir_out = SV.reference(oracle, W, r, dtype, wname, c)
                if c in ("nan_corner", "nan_last"):
                    fwd, inv = SV.reference_one_level(oracle, W, r, dtype, wname, c)
                missed = missed or any(o is not None and SV.condition(c, o, t and not SV.ENTRIES[r.entry].synthesis, wname == "haar", d) is not None
                                       for t, o, d in ((True, fwd, False), (False, inv, False), (False, dir_out, True)))
        assert missed, (n, c, "meets its condition: take it out of SKIPS")


# ---- coverage of the kernel names ------------------------------------------------------------------------------------------------
def _source_names():
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        with open(path) as f:
            for name in _re_name.findall(f.read()):
                found.setdefault(name, os.path.basename(path))
    return found


def test_every_reported_kernel_name_has_a_recipe():
    found = _source_names()
    assert len(found) > 60, sorted(found)
    have = SV.kernel_names()
    missing = sorted(n for n in found if n not in have and n not in SV.ELSEWHERE and n not in SV.NOT_KERNELS)
    assert not missing, "kernel names without a recipe in tests/special_values_cases.py: %s" % [(n, found[n]) for n in missing]
    # nothing names a kernel the sources no longer contain
    text = "".join(open(p).read() for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    stale = sorted(n for n in have | set(SV.ELSEWHERE) | set(SV.NOT_KERNELS) | set(SV.ZERO_SIGN_FREE) if '"%s"' % n not in text)
    assert not stale, stale
    assert not (have & set(SV.ELSEWHERE)) and not (have & set(SV.NOT_KERNELS))
    rows = [(r.entry, tuple(sorted(r.opts.items())), r.shape, r.L, r.wavelets, r.dtypes) for r in SV.RECIPES]
    assert len(set(rows)) == len(rows) and len({r.name for r in SV.RECIPES}) == len(SV.RECIPES)
    assert all(r.kfwd or r.kinv for r in SV.RECIPES)
    assert all(reason for reason in SV.ZERO_SIGN_FREE.values())


def test_design_tables_match():
    """DESIGN.md "Special values" lists the kernels of ZERO_SIGN_FREE and the pairs of SKIPS, no more and no fewer"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        sec = f.read().split("## 23. Special values")[1]
    rows = re.findall(r"^\| `([A-Za-z0-9_]+)` \| (?:`([a-z_]+)` \| )?", sec, re.M)
    assert {k for k, c in rows if not c and k.startswith("k_")} == set(SV.ZERO_SIGN_FREE)
    assert {(k, c) for k, c in rows if c} == set(SV.SKIPS)


def test_recipes_stay_small():
    for r in SV.RECIPES:
        assert int(np.prod(r.shape)) <= 2048 * 512, r.name
        assert r.entry in SV.ENTRIES and set(r.dtypes) <= set(SV.BOTH) and r.wavelets


# ---- the comparison --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_compare_on_hand_made_arrays(dtype):
    t = np.finfo(dtype).tiny
    sub = dtype(t / 8)
    want = np.array([1.0, sub, np.nan, np.inf, 0.0, -0.0, -2.5, -np.inf], dtype=dtype)
    SV.compare(want.copy(), want)
    SV.compare(want.copy(), want, zero_sign=False)

    def changed(i, v):
        g = want.copy()
        g[i] = v
        return g

    for zs in (True, False):
        assert "values differ" in SV.mismatch(changed(1, 0.0), want, zs)                 # a flushed subnormal
        assert "values differ" in SV.mismatch(changed(1, sub * 2), want, zs)             # ... or one a quantum step off
        assert "values differ" in SV.mismatch(changed(3, -np.inf), want, zs)             # an Inf of the wrong sign
        assert "values differ" in SV.mismatch(changed(4, sub), want, zs)                 # a zero that became non-zero
        assert "values differ" in SV.mismatch(changed(6, 0.0), want, zs)                 # a non-zero that became zero
        g = want.copy()
        g[2], g[0] = 1.0, np.nan                                                          # a moved NaN
        assert "NaN masks" in SV.mismatch(g, want, zs)
        assert "NaN masks" in SV.mismatch(changed(0, np.nan), want, zs)                  # a spread NaN
        assert "NaN masks" in SV.mismatch(changed(2, np.inf), want, zs)                  # a lost NaN
        # a NaN of another payload and sign
        g = want.copy()
        SV.bits(g)[2] = SV.bits(np.array([-np.nan], dtype=dtype))[0] | 0x1234
        assert np.isnan(g[2]) and SV.bits(g)[2] != SV.bits(want)[2]
        SV.compare(g, want, zs)
    # -0.0 for +0.0 and the other way round: only without zero_sign
    for i, v in ((4, -0.0), (5, 0.0)):
        assert "values differ" in SV.mismatch(changed(i, v), want, True)
        SV.compare(changed(i, v), want, zero_sign=False)
    with pytest.raises(AssertionError):
        SV.compare(changed(4, -0.0), want)
    assert "shape" in SV.mismatch(want[:4], want)


@pytest.mark.parametrize("dtype", [SV.F32, SV.F64])
def test_compare_rejects_a_flushed_straddle_output(W, oracle, dtype):
    """the stand-in for a flushing tier: the oracle's straddle output with its subnormals set to zero of the same sign"""
    r = next(q for q in SV.RECIPES if q.name == "tail2")
    x, fwd, inv_in, inv = SV.reference(oracle, W, r, dtype, "db4", "straddle")[:4]
    for out in (fwd, inv):
        flushed = np.where(np.abs(out) < np.finfo(out.dtype).tiny, np.copysign(0, out), out).astype(out.dtype)
        assert (flushed != out).sum() >= 0.05 * out.size
        for zs in (True, False):
            assert "values differ" in SV.mismatch(flushed, out, zs)
        SV.compare(out.copy(), out)


# ---- the float modes of the kernel descriptors -----------------------------------------------------------------------------------
def _isa():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import isa_check
    return isa_check


@pytest.mark.parametrize("lib", LIBS, ids=[os.path.basename(p) for p in LIBS])
def test_every_kernel_descriptor_keeps_denormals(lib):
    if not os.path.exists(lib):
        pytest.skip("library not built")
    m = _isa()
    seen, bad = 0, []
    with tempfile.TemporaryDirectory(prefix="wl_sv_") as tmp:
        for co in m.extract_code_objects(lib, tmp):
            out = subprocess.run([os.path.join(m.LLVM, "llvm-objdump"), "-D", "-j", ".rodata", co], check=True, capture_output=True,
                                 text=True).stdout
            for block in out.split(".amdhsa_kernel ")[1:]:
                block = block.split(".end_amdhsa_kernel")[0]
                seen += 1
                modes = dict(re.findall(r"\.amdhsa_float_denorm_mode_(32|16_64)\s+(\d+)", block))
                if modes != {"32": "3", "16_64": "3"}:
                    bad.append((block.split()[0], modes))
    assert not bad, bad[:10]
    stems = SV.kernel_names()
    assert seen >= len(stems), (seen, len(stems))
    print("%s: %d kernel descriptors, all with denorm modes 3 / 3" % (os.path.basename(lib), seen))
