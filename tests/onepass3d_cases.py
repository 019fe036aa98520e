"""Case table of the one-pass 3-D level tests (test_gpu_parity.py: test_3d_one_pass_level, test_3d_inverse_one_pass_level) and
the kernel instance each case reaches.

The launchers pick one template instance per level from the level's line length n0 (dim 1): k_fwd3d_one<T, RPL, F, NW>
(launch_fwd3d_f, wl_fwd3d.hip) and k_inv3d_one<T, RPL, F, NW> (launch_inv3d_f, wl_inv3d.hip).  The few lines below restate that
choice, so that test_onepass3d_coverage.py can check on the CPU that every instance in the built library is reached by a row that
the GPU tests compare with the oracle.  What the test sees of a call is its first forward level / its last inverse level: the
level of the full box, so the instance of a row is the instance of its full shape.
"""

# rows (n0, n1, n2), L.  Per row and filter the tests run the two-pass tier (compared with the oracle) and the one-pass kernel with
# every segment length (compared with the two-pass tier, bit for bit).
FWD_CASES = (
    ((256, 16, 16), 1), ((128, 32, 16), 1), ((256, 32, 48), 2), ((512, 16, 20), 1), ((1024, 16, 16), 2), ((256, 64, 32), 3),
    ((512, 64, 16), 1), ((128, 64, 64), 2),
    # lines that do not fill the last wave, 8-byte lanes on two to eight waves, dim-2 / dim-3 extents that are not multiples of
    # 8 / 4 (the last segment / tile overlaps its neighbour)
    ((200, 24, 20), 1), ((240, 40, 16), 2), ((320, 16, 16), 1), ((72, 16, 16), 1), ((1000, 16, 16), 1), ((136, 48, 24), 1),
    ((300, 16, 16), 1), ((180, 24, 20), 1), ((900, 16, 16), 1), ((256, 20, 18), 1), ((200, 30, 22), 1), ((304, 36, 28), 2),
    ((128, 70, 26), 1),
    # 10 taps on 4 and 8 waves with segments of 30 .. 60 columns (more than one group of U = 5 steps: consecutive steps across a
    # group boundary must not share an LDS exchange buffer)
    ((1024, 48, 16), 1), ((900, 40, 16), 1), ((300, 40, 16), 1),
)
INV_CASES = (
    ((256, 16, 16), 1), ((128, 32, 16), 1), ((256, 32, 48), 2), ((512, 16, 20), 1), ((1024, 16, 16), 2), ((256, 64, 32), 3),
    ((512, 64, 16), 1), ((128, 64, 64), 2), ((200, 24, 20), 1), ((240, 40, 16), 2), ((72, 16, 16), 1), ((1000, 16, 16), 1),
    ((300, 16, 16), 1), ((256, 20, 18), 1), ((200, 30, 22), 1), ((128, 70, 26), 1),
    # 8-byte Float32 lanes on two and eight waves
    ((180, 24, 20), 1), ((900, 16, 16), 1),
)

FWD_FILTERS = ("haar", "db2", "db3", "db4", "db5", "sym5")
INV_FILTERS = ("haar", "db2", "db3", "db4", "db5")
TAPS = {"haar": 2, "db2": 4, "db3": 6, "db4": 8, "db5": 10, "sym5": 10}
ESIZE = {"float": 4, "double": 8}

# the segment lengths the tests request (WL_3D_ONE_TJ; WL_3D_ONE_WAVES = 0 keeps them)
FWD_TJ = (64, 8, 16, 32)


def fwd3d_rpl(n0, esize):
    if n0 < 32 or n0 > 1024:
        return 0
    if esize == 4 and n0 > 128 and n0 % 8 == 0:
        return 4
    return 2 if n0 % 4 == 0 else 0


def waves(n0, rpl):
    w = 1
    while 64 * rpl * w < n0:
        w *= 2
    return w


def inv3d_rpl(n0, esize):
    if n0 < 32 or n0 > 1024:
        return 0
    if esize == 8 and n0 > 512:
        return 0
    if esize == 4 and n0 > 128 and n0 % 8 == 0:
        return 4
    return 2 if n0 % 4 == 0 else 0


def fwd_instance(t, F, n0):
    """-> (t, RPL, F, NW) of k_fwd3d_one for a level with lines of n0, or None where the kernel does not take the filter"""
    if F == 10:
        if t != "float" or n0 % 4 or not fwd3d_rpl(n0, 4):
            return None
        return (t, 2, F, waves(n0, 2))
    rpl = fwd3d_rpl(n0, ESIZE[t])
    return (t, rpl, F, waves(n0, rpl)) if rpl else None


def inv_instance(t, F, n0):
    if F > 8:
        return None
    rpl = inv3d_rpl(n0, ESIZE[t])
    return (t, rpl, F, waves(n0, rpl)) if rpl else None


def fwd_segment(n1, F, tj):
    """launch_fwd3d_f's segment length TJ for a requested tj with WL_3D_ONE_WAVES = 0 (steps per segment: TJ / 2)"""
    rs = 8 if F <= 8 else 10
    TJ = max(rs, tj // rs * rs)
    while TJ > rs and TJ > n1:
        TJ -= rs
    t = TJ
    while t >= rs and t >= TJ - 2 * rs:
        if n1 % t == 0:
            return t
        t -= rs
    return TJ


def fwd_cases_by_instance():
    """-> {instance: [(shape, L, filter, TJ)]} over both element types (dtype name as in the kernel: float / double)"""
    out = {}
    for shape, L in FWD_CASES:
        for t in ("float", "double"):
            for f in FWD_FILTERS:
                inst = fwd_instance(t, TAPS[f], shape[0])
                if inst is not None:
                    out.setdefault(inst, []).extend((shape, L, f, fwd_segment(shape[1], TAPS[f], tj)) for tj in FWD_TJ)
    return out


def inv_cases_by_instance():
    out = {}
    for shape, L in INV_CASES:
        for t in ("float", "double"):
            for f in INV_FILTERS:
                inst = inv_instance(t, TAPS[f], shape[0])
                if inst is not None:
                    out.setdefault(inst, []).append((shape, L, f))
    return out
