"""threshold_batch_ (wl_threshold_batch, wl_threshold_biggest_batch; W.threshold_batch_ / W.threshold_batch): everything that can be
checked without a device.

- the two symbols in the header, in _lib.SIGNATURES with the prototype's arity and pointer / scalar positions, and in `nm -D` of
  both libraries; a C99 translation unit that references them compiles against the header;
- the status codes whose rules need no device, in the documented order (threshold_batch_cases.RULES_EW / RULES_BIG);
- the TypeErrors of the Python mirror, raised before any device call;
- the shared cases are what the GPU tests need them to be.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import threshold_batch_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "wavelets_mi355x.h")
SYMS = ("wl_threshold_batch", "wl_threshold_biggest_batch")
# (the per-unit arrays are device pointers: bound as addresses)
C2CTYPES = {"wl_ctx *": C.c_void_p, "void *": C.c_void_p, "const double *": C.c_void_p, "const int64_t *": C.c_void_p, "int": C.c_int,
            "int64_t": C.c_int64, "double": C.c_double}


def _prototype(sym):
    hdr = open(HDR).read()
    params = re.search(r"WL_API int %s\((.*?)\);" % sym, hdr, re.S).group(1)
    out = []
    for p in params.split(","):
        p = " ".join(p.split())
        m = re.match(r"(.*?)(\w+)$", p)
        out.append((m.group(1).strip(), m.group(2)))
    return out


def test_symbols_in_header_signatures_and_both_libraries(W):
    from wavelets_jl_amd import _lib
    lib = _lib.load()
    for s in SYMS:
        proto = _prototype(s)
        assert s in _lib.SIGNATURES and _lib.SIGNATURES[s][0] is C.c_int
        argtypes = _lib.SIGNATURES[s][1]
        assert len(proto) == len(argtypes), s
        for k, ((ctype, name), at) in enumerate(zip(proto, argtypes)):
            assert C2CTYPES[ctype] is at, (s, k, name, ctype, at)
        assert hasattr(lib, s)
    assert [n for _, n in _prototype("wl_threshold_batch")] == list(TC.BASE_EW) + ["stream"]
    assert [n for _, n in _prototype("wl_threshold_biggest_batch")] == list(TC.BASE_BIG) + ["stream"]
    for path in _lib.LIB_PATHS.values():
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert set(SYMS) <= set(re.findall(r" T (wl_[a-z0-9_]+)", out)), path
    # the order of the status codes, what is not validated and the tiers are part of the header comment
    flat = " ".join(open(HDR).read().replace("\n *", " ").split())
    assert ("WL_EINVAL_ARG (NULL ctx / x), WL_EINVAL_DTYPE, WL_EDIMS (n < 1, nunits < 1, unit_stride < n, nunits * unit_stride overflows or "
            "reaches 2^60), WL_EINVAL_ARG (th not a wl_thtype; host t < 0).") in flat
    assert "WL_EINVAL_ARG (NULL ctx / x), WL_EINVAL_DTYPE, WL_EDIMS (as above), WL_EINVAL_ARG (host m < 0), then WL_ENOMEM / WL_EHIP." in flat
    assert "device thresholds are NOT validated" in flat and "each entry clamped on the device to [0, n]" in flat
    for name in ("k_threshold_batch", "k_threshold_batch_wave", "k_thbig_lds", "k_thbig_stream", "k_thbig_split", "WL_THB_LDS_MAX", "WL_THB_SPLIT_N", "WL_THB_SPLIT_UNITS",
                 "WL_THB_CHUNK"):
        assert name in flat, name


def test_a_c99_translation_unit_compiles_against_the_header(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "wavelets_mi355x.h"\n'
                   "int use(wl_ctx *c, void *x, const double *t, const int64_t *m, void *s)\n"
                   "{ return wl_threshold_batch(c, WL_F32, x, 64, 3, 68, WL_TH_SOFT, 0.5, t, 1, s)\n"
                   "       + wl_threshold_biggest_batch(c, WL_F64, x, 64, 3, 68, 5, m, s); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def test_status_codes_in_order_through_a_dummy_context(W):
    """every row breaks one rule and every later one; the argument rules run before the context is touched, so a block of zero
    bytes serves as the context"""
    lib = W._lib.load()
    ST = W._lib.STATUS
    buf = (C.c_float * 16384)()
    dummy = (C.c_char * 4096)()
    named = {"CTX": C.cast(dummy, C.c_void_p), "P": C.cast(buf, C.c_void_p)}

    def call(fn, base, args):
        a = {**base, **args}
        return ST[fn(*[named.get(v, v) if isinstance(v, str) else v for v in a.values()], None)]

    for fn, base, rules in ((lib.wl_threshold_batch, TC.BASE_EW, TC.RULES_EW), (lib.wl_threshold_biggest_batch, TC.BASE_BIG, TC.RULES_BIG)):
        seen = []
        for status, args in TC.rows(rules):
            assert call(fn, base, args) == status, (fn.__name__, status, args)
            seen.append(status)
        for status, breakers in rules:
            for b in breakers:
                assert call(fn, base, b) == status, (fn.__name__, status, b)
        assert [s for k, s in enumerate(seen) if k == 0 or seen[k - 1] != s] == [TC.ARG, TC.DTYPE, TC.EDIMS, TC.ARG]
    # Pos / Neg take no threshold: a negative t is not looked at; a device threshold array switches the host check off.  Both get past
    # the argument rules -- to the dummy context, whose device is not there
    rows = TC.rows(TC.RULES_EW)
    assert (TC.DTYPE, dict(dtype=7, n=0, th=6)) in rows and (TC.EDIMS, dict(n=0, th=6)) in rows


def test_python_type_errors_need_no_device(W):
    import torch

    def cpu(*shape, dtype=torch.float32):
        return torch.zeros(*reversed(shape), dtype=dtype).permute(*reversed(range(len(shape))))

    x = cpu(100, 3)
    for f in (W.threshold_batch_, W.threshold_batch):
        for m in (2.5, None, torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32)):
            with pytest.raises(TypeError, match=re.escape("threshold!(x, BiggestTH(), m::Int)")):
                f(x, W.BiggestTH(), m)
        for th in (W.PosTH(), W.NegTH()):
            for t in (1.0, 0, torch.zeros(3, dtype=torch.float64)):
                with pytest.raises(TypeError, match="takes no threshold"):
                    f(x, th, t)
        for th in (W.HardTH(), W.SoftTH(), W.SemiSoftTH(), W.SteinTH()):
            with pytest.raises(TypeError, match="t is required"):
                f(x, th)
            with pytest.raises(TypeError, match="per-unit thresholds are a Float64 tensor"):
                f(x, th, torch.zeros(3, dtype=torch.int64))
            with pytest.raises(AssertionError, match="t >= 0"):
                f(x, th, -1.0)
            with pytest.raises(AssertionError, match="t >= 0"):
                f(x, th, float("nan"))
        with pytest.raises(AssertionError, match="m >= 0"):
            f(x, W.BiggestTH(), -1)
        for bad in (None, "hard", W.HardTH, W.THType()):
            with pytest.raises(TypeError, match="unknown threshold type"):
                f(x, bad, 1.0)
        with pytest.raises(TypeError, match=f.__name__ + " is not defined for complex arrays"):
            f(x.to(torch.complex64), W.HardTH(), 1.0)
        with W.complex_arrays():
            with pytest.raises(TypeError, match=f.__name__ + " is not defined for complex arrays"):
                f(x.to(torch.complex64), W.BiggestTH(), 3)
        assert f.__name__ in W.__all__
    # valid arguments get as far as the device check, here without a device
    if not torch.cuda.is_available():
        for call in (lambda: W.threshold_batch_(x, W.HardTH(), 1), lambda: W.threshold_batch_(x, W.BiggestTH(), 7),
                     lambda: W.threshold_batch(x, W.PosTH()), lambda: W.threshold_batch_(np.zeros((4, 3)), W.NegTH())):
            with pytest.raises(W.HIPError):
                call()


def test_the_shared_cases_are_what_the_gpu_tests_need(oracle):
    for dt in TC.DTYPES:
        assert TC.LDS_MAX[dt] * np.dtype(dt).itemsize == 32768
        u = TC.units(100, 5, dt)
        assert u.shape == (5, 100) and u.dtype == dt and np.array_equal(u[:3], TC.units(100, 3, dt))
        assert len(np.unique(np.abs(u[0]))) < 40 and len(np.unique(np.abs(u[1]))) == 100           # ties in the even units only
        t = TC.tie_units(100, dt)
        assert set(np.unique(np.abs(t[:2]))) == {0.0, 1.0, 2.0} and np.signbit(t[0][t[0] == 0]).any() and len(np.unique(t[2])) == 1
        nf = TC.nonfinite_units(100, dt)
        assert not np.isnan(nf[:2]).any() and np.isinf(nf[:2]).any() and np.isnan(nf[2]).sum() == 3 and np.isnan(nf[3]).sum() == 3
        assert ((np.abs(nf[0]) > 0) & (np.abs(nf[0]) < np.finfo(dt).tiny)).sum() == 6
        # the oracle states the tie rule of the device calls: lower index first
        for unit in (t[0], t[2], u[0], nf[1], TC.split_run_unit(dt)):
            for m in (0, 1, unit.size // 3, unit.size - 1, unit.size):
                assert np.array_equal(TC.ibits(oracle.threshold(unit, "biggest", m=m)), TC.ibits(TC.biggest_ref(unit, m))), (dt, m)
        r = TC.split_run_unit(dt)
        assert r.size == 5000 and (np.abs(r) == 1).sum() == 3800 and (np.abs(r) < 1).sum() == 300 and abs(r[900]) == 1 == abs(r[4699])
        buf = TC.layout(u[:3], 103, dt)
        assert buf.size == 2 * TC.GUARD + 3 * 103 and (TC.ibits(buf) == TC.SENT[dt]).sum() == 2 * TC.GUARD + 3 * 3
    assert [TC.ew_kernel(*a) for a in ((256, 3, 257, False), (257, 3, 258, False), (5, 1, 5, True), (5, 3, 5, False), (5, 3, 5, True))] == [
        "k_threshold_batch_wave", "k_threshold_batch", "k_threshold_batch", "k_threshold_batch", "k_threshold_batch_wave"]
    assert TC.scalar_ms(100) == [0, 1, 50, 99, 100, 105] and TC.unit_ms(100, 5) == [0, 100, 101, -3, 50]
    assert {k: v[0] for k, v in TC.TIERS.items()} == {"lds": "k_thbig_lds", "stream": "k_thbig_stream", "split": "k_thbig_split"}
