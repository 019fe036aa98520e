"""The table of tests/batch_limits_cases.py without a device: every row crosses the limit it names under the launch rules restated
there, the tiled expected buffers equal the plain loop of oracle calls over the units, and no batched function of the ABI is
without a row."""
import os
import re

import numpy as np
import pytest

import batch_limits_cases as BL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# rows whose reference is the CPU oracle (the best-basis rows take the single device call: test_gpu_batch_limits.py alone runs them)
ORACLE_ROWS = [r["id"] for r in BL.ROWS if r["kind"] != "bestbasis"]


def test_periods_are_coprime_to_every_limit():
    """61 is coprime to every limit; 7 to every limit of a row that takes per-unit parameters (32767 = 7 * 31 * 151: the complex
    batches, which have none)"""
    for r in BL.ROWS:
        lims = {BL.crossing(r)[1]}
        if r["rule"][0] == "sweep":
            lims.add(BL.modwt_lds_shape(r["n"], 1 << 40, BL.is_vec(r), np.dtype(BL.DT[r["dtype"]]).itemsize, BL.CU_HOST)[2])
        if r["rule"][0] == "blocks":
            lims = {65535, 36004}
        if r["rule"][0] == "planes":                         # the even groups the TI batch cuts its planes into, in units where whole
            planes = BL.crossing(r)[0]
            lims.add(-(-planes // 2))
        for lim in lims:
            assert np.gcd(lim, BL.D) == 1, (r["id"], lim)
            assert not BL.params_of(r) or np.gcd(lim, BL.P) == 1, (r["id"], lim)


@pytest.mark.parametrize("rid", [r["id"] for r in BL.ROWS])
def test_row_crosses_its_limit(rid):
    r = BL.BY_ID[rid]
    over, limit = BL.crossing(r)
    assert over > limit, (rid, over, limit)
    assert over <= limit + max(limit // 8, 600), (rid, "far more than the limit needs", over, limit)
    what = r["rule"][0]
    B = BL.units_of(r)
    if what == "group":
        # the group the launcher forms is the limit itself (no workspace cap halves it at these sizes), so a second group runs
        G = BL.group_size(B, limit, int(r["opts"].get("WL_MODWT_BATCH_GROUP", 0)))
        assert G == limit and -(-B // G) == 2
    if what == "sweep":
        _, grid, upw = BL.modwt_lds_shape(r["n"], over, BL.is_vec(r), np.dtype(BL.DT[r["dtype"]]).itemsize, BL.CU_HOST)
        assert grid == BL.CU_HOST * 8 and over > grid * upw                  # a second sweep, and it starts in a full workgroup
        assert upw == (1 if "-one" in rid else (128 if BL.is_vec(r) else 32))
    if r["kind"] == "threshold":
        assert r["n"] > 256                                                  # (shorter units take the wave tier: UNREACHED)
        bx = BL.ext_blocks(r["n"], 4, BL.CU_HOST)
        assert bx * 65535 > BL.CU_HOST * 64                                  # the clamp of the grid's x is taken as well
    # the largest buffer of a row stays below 140 MB (its expected twin is built after the call: about 256 MB of device data in all)
    cols = {"modwt": r.get("L", 0) + 1, "imodwt": r.get("ncols", 1), "mra": r.get("ncols", 1), "cdwt": 2, "csplit": 2, "cmerge": 2}.get(r["kind"], 1)
    nbytes = B * (BL.unit_len(r) + r["pad"]) * cols * np.dtype(BL.DT[r["dtype"]]).itemsize
    assert nbytes < (140 << 20), (rid, nbytes)


@pytest.mark.parametrize("rid", ORACLE_ROWS)
def test_builder_is_the_plain_loop(oracle, W, rid):
    """B = 130: more than two periods of the units and eighteen of the parameters"""
    r = BL.BY_ID[rid]
    B = 130
    bufs = BL.build(r, oracle, W, B)
    want = BL.plain_loop(r, oracle, W, B)
    written = {k for k, b in bufs.items() if b["role"] in ("out", "inout")}
    assert written == set(want), (rid, written, set(want))
    for name in written:
        b = bufs[name]
        got = BL.tiled_host(b["table"], b["index"], b["stride"])
        assert got.dtype == want[name].dtype and np.array_equal(BL.ibits(got), BL.ibits(want[name])), (rid, name)
        m = b["table"].shape[1]
        body = BL.ibits(got)[BL.GUARD:BL.GUARD + B * b["stride"]].reshape(B, b["stride"])
        assert np.all(body[:, m:] == BL.SENT[got.dtype]) and np.all(BL.ibits(got)[:BL.GUARD] == BL.SENT[got.dtype])
    # the expected content separates the units: at least one distinct result per distinct input unit in the call's main buffer
    b = bufs[max(written, key=lambda k: bufs[k]["table"].shape[1])]
    rows = {b["table"][i].tobytes() for i in range(b["table"].shape[0])}
    assert len(rows) >= BL.D, (rid, "the expected units are not distinct", len(rows))


def batched_abi_functions():
    """every function of the header whose arguments include a count of units"""
    text = open(os.path.join(ROOT, "include", "wavelets_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = []
    for m in re.finditer(r"WL_API\s+[\w\s\*]+?\b(wl_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        names = re.findall(r"(\w+)\s*(?:,|$)", m.group(2).replace("\n", " "))
        if {"nunits", "nimages", "nvolumes", "ns", "nsignals"} & set(names):
            out.append(m.group(1))
    return out


def test_no_batched_abi_function_is_left_out():
    fns = batched_abi_functions()
    assert len(fns) >= 24 and "wl_modwt_mra_batch" in fns and "wl_dwtc_lifting_oop" in fns and "wl_dwt_filter" not in fns, fns
    covered = {r["fn"] for r in BL.ROWS} | {k for k in BL.UNREACHED if k.startswith("wl_") and ":" not in k}
    assert not [f for f in fns if f not in covered], "a batched ABI function without a row in batch_limits_cases.ROWS or an UNREACHED entry"
    assert all(isinstance(v, str) and len(v) > 20 for v in BL.UNREACHED.values())
