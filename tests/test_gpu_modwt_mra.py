"""modwt_mra / modwt_mra_batch on the device (wl_modwt_mra_batch, W.modwt_mra / W.modwt_mra_batch): the details D_1 .. D_L and the
smooth S_L of a batch of coefficient matrices.  Every result is compared with np.array_equal against the definition -- the CPU
oracle's imodwt of the unit with every column but one set to +0 (modwt_mra_cases.reference; the sign of a zero is not part of the
contract, so the comparison is by value).  Every shape runs on both tiers -- the LDS kernel where the unit fits, and the per-level
kernels under WL_MODWT_FUSED = 0 -- and the two must give the same bytes.  Shapes, units and references: modwt_mra_cases.
"""
import ctypes as C

import numpy as np
import pytest

import modwt_mra_cases as RC
from test_gpu_modwt_batch import SENT, _hip, coefs, filt, fits_lds, ibits, units_of

pytestmark = pytest.mark.gpu

TIERS = (("lds", {}), ("step", {"WL_MODWT_FUSED": 0}))
ELSEWHERE = ("db4", "sym5")


def run_tiers(W, cd, wt, ref, n, dtype, opts=None, label=()):
    """the analysis of the device coefficients cd on both tiers against ref (B, ncols, n); returns {tier: kernel}"""
    names, raw = {}, {}
    for tier, o in TIERS:
        with W.options(**{**o, **(opts or {})}):
            y = W.modwt_mra_batch(cd, wt)
            names[tier] = W.last_kernel()
        assert tuple(y.shape) == tuple(cd.shape) and W.is_julia_layout(y)
        got = units_of(W, y)
        assert np.array_equal(got, ref), (tier, names[tier], label, int((got != ref).sum()))
        raw[tier] = got.tobytes()
        assert names[tier] == ("k_modwt_mra_lds" if tier == "lds" and fits_lds(n, dtype) else "k_modwt_mra_step_b"), (tier, n, names[tier])
    assert raw["lds"] == raw["step"], ("the tiers differ", label)
    return names


def check(W, oracle, fname, n, B, dtype, L, opts=None):
    co = RC.forward(oracle, W, fname, n, B, dtype, L)
    ref = RC.reference(oracle, W, fname, n, B, dtype, L)
    return run_tiers(W, coefs(W, co), filt(W, fname), ref, n, dtype, opts, (fname, n, B, L))


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_wrap_around_on_tiny_units(gpu, W, oracle, dtype):
    """n in {2, 3, 8, 12}: the tap reach 2^(j-1) (F - 1) goes round the unit several times for the long filters; and n = 3 with
    eight columns, where the stride itself exceeds n many times over (ncols is not bounded by log2 n)"""
    for n, B, L in RC.shapes(dtype)["wrap"]:
        for fname in RC.FILTERS:
            check(W, oracle, fname, n, B, dtype, L)
    n, B, L = RC.DEEP
    co = RC.deep_coefficients(dtype)
    for fname in RC.FILTERS:
        wt = filt(W, fname)
        ref = np.stack([RC.mra_of(oracle, wt.qmf, co[u]) for u in range(B)])
        run_tiers(W, coefs(W, co), wt, ref, n, dtype, None, (fname, "deep"))


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_several_planes_per_workgroup(gpu, W, oracle, dtype):
    """n = 64 and n = 100: a workgroup of the LDS tier takes several whole planes; (L + 1) B is no multiple of its share, so one
    workgroup holds planes of two columns that start at different levels, and the last one is short; and a batch of one, whose
    seven planes of seven depths share a workgroup"""
    for n, B, L in RC.shapes(dtype)["packing"]:
        for fname in ELSEWHERE:
            check(W, oracle, fname, n, B, dtype, L)


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_tier_boundary(gpu, W, oracle, dtype):
    """the longest unit of the LDS tier and one 16-byte vector more: the two sides take different tiers"""
    (n0, B, L), (n1, _, _) = RC.shapes(dtype)["boundary"]
    for fname in ELSEWHERE:
        below = check(W, oracle, fname, n0, B, dtype, L)
        above = check(W, oracle, fname, n1, B, dtype, L)
        assert below["lds"] == "k_modwt_mra_lds" and above["lds"] == "k_modwt_mra_step_b"


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_long_units(gpu, W, oracle, dtype):
    for n, B, L in RC.shapes(dtype)["long"]:
        for fname in ELSEWHERE:
            assert check(W, oracle, fname, n, B, dtype, L) == {"lds": "k_modwt_mra_step_b", "step": "k_modwt_mra_step_b"}


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_groups_change_no_bit(gpu, W, oracle, dtype):
    """five units in groups of two (WL_MODWT_BATCH_GROUP = 2): two full groups and a short one on the per-level tier"""
    for n, B, L in RC.shapes(dtype)["groups"]:
        for fname in ELSEWHERE:
            check(W, oracle, fname, n, B, dtype, L, opts={"WL_MODWT_BATCH_GROUP": 2})
            check(W, oracle, fname, n, B, dtype, L)


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_unaligned_and_padded_tensors_write_nothing_else(gpu, W, oracle, dtype):
    """n in {129, 1000}, B = 3, ldw = n + 1, ldo = n + 3, unit strides ld * ncols + 5, every buffer one element off a 16-byte
    boundary: the padding rows, the padding between units and the guard bands of out keep the sentinel's bits, and xw comes back
    unchanged"""
    import torch
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    idt = torch.int32 if dtype == np.float32 else torch.int64
    sent = np.array([SENT[dtype]], dtype=np.uint32 if dtype == np.float32 else np.uint64).view(np.int32 if dtype == np.float32 else np.int64)[0]
    G = 33                                                                # guard elements: the bases are odd
    for n, B in RC.UNALIGNED:
        L = 3
        nc = L + 1
        ldw, ldo = n + 1, n + 3
        ws, ous = ldw * nc + 5, ldo * nc + 5
        for fname in ELSEWHERE:
            wt = filt(W, fname)
            co = RC.forward(oracle, W, fname, n, B, dtype, L)
            ref = RC.reference(oracle, W, fname, n, B, dtype, L)
            wbuf = torch.full((G + B * ws + G,), int(sent), dtype=idt, device=gpu).view(tdt)
            wv = wbuf.as_strided((n, nc, B), (1, ldw, ws), G)
            wv.copy_(coefs(W, co))
            torch.cuda.synchronize()
            before = ibits(wbuf.cpu().numpy()).copy()
            for tier, o in TIERS:
                ybuf = torch.full((G + B * ous + G,), int(sent), dtype=idt, device=gpu).view(tdt)
                yv = ybuf.as_strided((n, nc, B), (1, ldo, ous), G)
                with W.options(**o):
                    out = W.modwt_mra_batch(wv, wt, y=yv)
                    assert W.last_kernel() == ("k_modwt_mra_lds" if tier == "lds" else "k_modwt_mra_step_b")
                assert out.data_ptr() == yv.data_ptr() == ybuf.data_ptr() + G * ybuf.element_size()
                torch.cuda.synchronize()
                hy = ybuf.cpu().numpy()
                body = hy[G: G + B * ous].reshape(B, ous)
                mats = body[:, : ldo * nc].reshape(B, nc, ldo)
                assert np.array_equal(mats[:, :, :n], ref), (tier, fname, n)
                rest = np.concatenate((hy[:G], mats[:, :, n:].ravel(), body[:, ldo * nc:].ravel(), hy[G + B * ous:]))
                assert np.all(ibits(rest) == SENT[dtype]), ("padding written", tier, fname, n)
                assert np.array_equal(ibits(wbuf.cpu().numpy()), before), ("xw changed", tier, fname, n)


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_one_matrix_one_column_and_a_given_result(gpu, W, oracle, dtype):
    """modwt_mra of a matrix is unit 0 of the batch; a single column is copied ("copy"); y= dense and padded is filled in place;
    a row-major tensor is copied once"""
    import torch
    n, B, L = 1000, 3, 4
    wt = filt(W, "db4")
    co = RC.forward(oracle, W, "db4", n, B, dtype, L)
    ref = RC.reference(oracle, W, "db4", n, B, dtype, L)
    cd = coefs(W, co)
    for tier, o in TIERS:
        with W.options(**o):
            one = W.modwt_mra(cd[:, :, 0], wt)
            assert W.last_kernel() == ("k_modwt_mra_lds" if tier == "lds" else "k_modwt_mra_step_b")
        assert tuple(one.shape) == (n, L + 1)
        torch.cuda.synchronize()
        assert np.array_equal(W.to_host(one).T, ref[0]), tier
    m = W.modwt(W.to_device(RC.units(n, B, dtype)[1]), wt, L)                 # what a user holds: the single transform's matrix
    torch.cuda.synchronize()
    assert np.array_equal(W.to_host(W.modwt_mra(m, wt)).T, ref[1])
    col = coefs(W, co[:, L:, :])                                             # ncols = 1: the smooth is the scaling column
    yc = W.modwt_mra_batch(col, wt)
    assert W.last_kernel() == "copy" and np.array_equal(units_of(W, yc), co[:, L:, :])
    # y = dense, then padded
    y = W.similar(cd)
    assert W.modwt_mra_batch(cd, wt, y=y) is y and np.array_equal(units_of(W, y), ref)
    ld, us = n + 8, (n + 8) * (L + 1) + 16
    buf = torch.zeros(B * us, dtype=cd.dtype, device=gpu)
    yp = buf.as_strided((n, L + 1, B), (1, ld, us))
    assert W.modwt_mra_batch(cd, wt, y=yp).data_ptr() == buf.data_ptr() and np.array_equal(units_of(W, yp), ref)
    hb = buf.cpu().numpy().reshape(B, us)
    assert not hb[:, ld * (L + 1):].any() and not hb[:, : ld * (L + 1)].reshape(B, L + 1, ld)[:, :, n:].any()
    rowmajor = torch.from_numpy(np.ascontiguousarray(co.transpose(2, 1, 0))).to(gpu)      # strides (ncols * B, B, 1)
    assert not W.is_julia_layout(rowmajor) and np.array_equal(units_of(W, W.modwt_mra_batch(rowmajor, wt)), ref)
    with pytest.raises(W.DimensionMismatch):
        W.modwt_mra_batch(cd, wt, y=W.similar(cd)[:, :L, :])
    with pytest.raises(W.ArgumentError, match="y must be column-major"):
        W.modwt_mra_batch(cd, wt, y=torch.empty((n, L + 1, B), dtype=cd.dtype, device=gpu))
    with pytest.raises(W.ArgumentError, match="WL_EALIAS"):                   # no in-place form
        W.modwt_mra_batch(cd, wt, y=cd)


def test_status_codes_in_order_with_a_live_context(gpu, W):
    """every row of the rule table, each breaking one rule and every later one, and each rule alone"""
    import torch
    lib = W._lib.load()
    ST = W._lib.STATUS
    hctx, st = W.transforms._context(gpu)
    p, q = torch.zeros(16384, dtype=torch.float32, device=gpu), torch.zeros(16384, dtype=torch.float32, device=gpu)
    qmf = (C.c_double * 64)(*([0.5] * 64))
    named = {"CTX": hctx, "P": C.c_void_p(p.data_ptr()), "Q": C.c_void_p(q.data_ptr()), "Q+32": C.c_void_p(q.data_ptr() + 32 * 4), "QMF": qmf}

    def call(args):
        a = {**RC.BASE, **args}
        return ST[lib.wl_modwt_mra_batch(*[named.get(v, v) if isinstance(v, str) else v for v in a.values()], st)]

    assert call({}) == "WL_OK"
    for status, args in RC.rows(RC.RULES):
        assert call(args) == status, (status, args)
    for status, breakers in RC.RULES:
        for b in breakers:
            assert call(b) == status, (status, b)
    torch.cuda.synchronize()


# ---- hipGraph ----------------------------------------------------------------------------------------------------------------------
def test_hipgraph_capture_one_node_or_a_chain_and_replays(gpu, W, oracle):
    """1024 x 5, L = 4, captured on one stream after reserve_workspace: the LDS tier is a single kernel node, the per-level tier a
    chain of 2 L kernel nodes (every node has at most one predecessor and one successor, edges = nodes - 1); replays on new
    coefficients in the same buffers give the reference"""
    import torch
    n, B, L = RC.shapes(np.float32)["groups"][0]
    wt = filt(W, "db4")
    co = RC.forward(oracle, W, "db4", n, B, np.float32, L)
    ref = RC.reference(oracle, W, "db4", n, B, np.float32, L)
    inputs = [(co, ref), (np.ascontiguousarray(co[::-1]), np.ascontiguousarray(ref[::-1]))]       # the units in reverse order: new values
    hip = _hip()
    for tier, o in TIERS:
        with W.options(**o):
            xw = coefs(W, np.zeros_like(co))
            y = W.similar(xw)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                W.reserve_workspace(xw, full=True)
                assert W.workspace_held() >= 2 * xw.numel() * 4
                hctx, _ = W.transforms._context(gpu)                         # the context of the capture stream
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                W.modwt_mra_batch(xw, wt, y=y)
            for c, r in inputs:
                xw.copy_(coefs(W, c))
                y.zero_()
                graph.replay()
                assert np.array_equal(units_of(W, y), r), tier
            del graph
            # the topology, through the runtime's own capture of the same call
            lib = W._lib.load()
            q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
            st = C.c_void_p(s.cuda_stream)
            g = C.c_void_p()
            torch.cuda.synchronize()
            assert hip.hipStreamBeginCapture(st, 2) == 0                    # hipStreamCaptureModeRelaxed
            rc = lib.wl_modwt_mra_batch(hctx, 0, C.c_void_p(y.data_ptr()), n, n * (L + 1), C.c_void_p(xw.data_ptr()), n, n * (L + 1), n, L + 1, B,
                                        q.ctypes.data_as(C.POINTER(C.c_double)), len(q), st)
            assert hip.hipStreamEndCapture(st, C.byref(g)) == 0 and rc == 0
            nn, ne = C.c_size_t(0), C.c_size_t(0)
            assert hip.hipGraphGetNodes(g, None, C.byref(nn)) == 0 and hip.hipGraphGetEdges(g, None, None, C.byref(ne)) == 0
            want = 1 if tier == "lds" else 2 * L
            assert nn.value == want and ne.value == want - 1, (tier, nn.value, ne.value)
            if ne.value:
                src, dst = (C.c_void_p * ne.value)(), (C.c_void_p * ne.value)()
                assert hip.hipGraphGetEdges(g, src, dst, C.byref(ne)) == 0
                assert len(set(src)) == len(set(dst)) == ne.value, "a node with two successors or two predecessors"
            assert hip.hipGraphDestroy(g) == 0
