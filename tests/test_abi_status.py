"""The order of the status codes of the entry points listed in abi_status_cases.py: every row breaks one rule and every later one
and must return the status of the rule it names.

- host: the rows whose rule comes before the entry point makes the context's device current, through a block of zero bytes as
  the context and host buffers (as test_wpt_batch_host.py does);
- gpu: every row through a live context, the buffers being device tensors of the base call's sizes.  Every row fails its
  validation, so nothing is launched.
"""
import ctypes as C

import numpy as np
import pytest

import abi_status_cases as AC
import lifting_schemes as LS

NBYTES = 16384                 # per data buffer: 8 x 8 x 8 Float64 values of two units twice over


def _supplies(W, origin):
    """what the names in capitals of the table stand for; the second value keeps the memory alive"""
    keep = []
    if origin == "host":
        bufs = [(C.c_char * NBYTES)() for _ in range(3)]
        ptrs = [C.cast(b, C.c_void_p) for b in bufs]
        ctx = C.cast((C.c_char * 4096)(), C.c_void_p)
        keep += bufs + [ctx]
        stream = None
    else:
        import torch
        dev = torch.device("cuda", 0)
        bufs = [torch.zeros(NBYTES, dtype=torch.uint8, device=dev) for _ in range(3)]
        ptrs = [C.c_void_p(b.data_ptr()) for b in bufs]
        ctx, stream = W.transforms._context(dev)
        keep += bufs
    sch = LS.scheme(W, "cdf97")
    iu, nc, sh, cf = sch.flatten()
    qmf = np.ascontiguousarray(W.wavelet(W.WT.db2).qmf, dtype=np.float64)
    badnc = np.array([0] + [2] * (len(nc) - 1), dtype=np.int32)
    tree = np.zeros(63, dtype=np.uint8)
    tree[:2] = 1
    badtree = np.zeros(63, dtype=np.uint8)
    badtree[1] = 1
    treeout, res = np.zeros(63, dtype=np.uint8), np.zeros(8, dtype=np.float64)
    keep += [iu, nc, sh, cf, qmf, badnc, tree, badtree, treeout, res]
    i32, f64, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    sup = {"CTX": ctx, "B0": ptrs[0], "B1": ptrs[1], "DRES": C.cast(ptrs[2], f64), "RES": res.ctypes.data_as(f64), "QMF": qmf.ctypes.data_as(f64),
           "NSTEPS": len(iu), "IU": iu.ctypes.data_as(i32), "NC": nc.ctypes.data_as(i32), "SH": sh.ctypes.data_as(i32),
           "CF": cf.ctypes.data_as(f64), "NORM1": sch.norm1, "NORM2": sch.norm2, "BADNC": badnc.ctypes.data_as(i32),
           "TREE": tree.ctypes.data_as(u8), "BADTREE": badtree.ctypes.data_as(u8), "TREEOUT": treeout.ctypes.data_as(u8)}
    return sup, stream, keep


def _run(W, origin):
    lib = W._lib.load()
    ST = W._lib.STATUS
    for sym, base, _ in AC.ENTRIES:                      # every base set has the prototype's arity and ends with the stream
        assert len(base) == len(W._lib.SIGNATURES[sym][1]) and base[-1] == ("stream", None), sym
    sup, stream, keep = _supplies(W, origin)
    i64 = C.POINTER(C.c_int64)
    seen, wrong = set(), []
    for rid, sym, args, status, live in AC.rows():
        seen.add(sym)
        if live and origin == "host":
            continue
        vals = []
        for a in args[:-1]:
            if isinstance(a, str):
                a = sup[a]
            elif isinstance(a, tuple):
                arr = np.array(a, dtype=np.int64)
                keep.append(arr)
                a = arr.ctypes.data_as(i64)
            vals.append(a)
        got = ST[getattr(lib, sym)(*vals, stream)]
        if got != status:
            wrong.append((rid, got))
    assert not wrong, wrong
    return seen


def test_status_codes_in_order_through_a_dummy_context(W):
    assert len(_run(W, "host")) == len(AC.ENTRIES)


@pytest.mark.gpu
def test_status_codes_in_order_through_a_live_context(W, gpu):
    assert len(_run(W, "device")) == len(AC.ENTRIES)
