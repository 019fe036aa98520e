"""The tall-tile instance of k_fwd2d_tileB (levels 3-4 of the 8192^2 transform: two fused levels, tiles of TR x 64 instead of
64 x 64) against the CPU oracle, bit for bit -- and, with WL_TILEB_TALL = 0, the 64 x 64 kernel on the same calls.

Shapes are rows x columns.  The smallest ones at which the new code can go wrong: one tile (both halos wrap onto the tile itself),
grids that take the plain tile map (a y count that is no multiple of four, an odd x count) and one that takes the XCD-compact map,
nine column tiles with the wrap in the last, rows that are a multiple of 64 but not of TR (the 64 x 64 kernel must take them), and
the default dispatch of a 2048 x 1024 block.  Every call is made twice into the same output."""
import numpy as np
import pytest

from conftest import rng_array

pytestmark = pytest.mark.gpu

TR = 256                                    # rows of the tall tile (wl_tile.hip)
FILTERS = ("haar", "db2", "db3", "db4", "sym5")     # F = 2, 4, 6, 8, 10
SMALL = {"WL_TILEB_MIN": 0, "WL_TILE": 0, "WL_M2D_MAX": 64}        # small blocks reach the kernel
CASES = [
    ((TR, 128), SMALL),                     # one tile in x
    ((2 * TR, 128), SMALL),                 # 2 x 2 tiles: plain map
    ((3 * TR, 256), SMALL),                 # odd count in x: plain map
    ((2 * TR, 256), SMALL),                 # 2 x 4 tiles: the XCD map's condition holds
    ((128, 576), SMALL),                    # nine column tiles, a wrap in the last (rows below TR: the 64 x 64 kernel)
    ((TR, 576), SMALL),                     # ... and on the tall tiles
    ((192, 128), SMALL),                    # rows a multiple of 64, not of 128 or TR: the 64 x 64 kernel
    ((2048, 1024), {}),                     # the default dispatch (128 tall tiles would leave CUs idle: the 64 x 64 kernel)
]


def _twice(W, x, wt, L):
    import torch
    y = W.similar(x)
    W.dwt_oop_(y, x, wt, L)
    W.dwt_oop_(y, x, wt, L)
    torch.cuda.synchronize()
    return W.to_host(y)


@pytest.mark.parametrize("shape,opts", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_tall_tiles_bitexact(gpu, W, oracle, shape, opts):
    xh = rng_array(shape, np.float32, 11 + sum(shape))
    x = W.to_device(xh)
    Lmax = W.maxtransformlevels(xh)
    for fname in FILTERS:
        wt = W.wavelet(getattr(W.WT, fname))
        for L in (2, 3, Lmax):              # the launch writes the last approximation into y / something follows it / full depth
            ye = oracle.dwt_filter(xh, wt.qmf, L)
            for tall in (1, 0):
                W.clear_options()
                for k, v in opts.items():
                    W.set_option(k, v)
                W.set_option("WL_TILEB_TALL", tall)
                y = _twice(W, x, wt, L)
                assert W.last_kernel() == "k_fwd2d_tileB", (shape, fname, L, tall, W.last_kernel())
                assert np.array_equal(y, ye), (shape, fname, L, tall, int((y != ye).sum()))


def test_default_dispatch_takes_the_kernel(gpu, W, oracle):
    xh = rng_array((2048, 1024), np.float32, 5)
    wt = W.wavelet(W.WT.db4)
    y = _twice(W, W.to_device(xh), wt, 2)
    assert W.last_kernel() == "k_fwd2d_tileB"
    assert np.array_equal(y, oracle.dwt_filter(xh, wt.qmf, 2))


def test_tall_tiles_replay_from_a_graph(gpu, W, oracle):
    import torch
    wt = W.wavelet(W.WT.db4)
    xin = [rng_array((256, 256), np.float32, 70 + k) for k in range(3)]
    s = torch.cuda.Stream()
    xg = W.to_device(xin[0])
    yg = W.similar(xg)
    with torch.cuda.stream(s):
        for k, v in SMALL.items():
            W.set_option(k, v)              # (options are per context = per stream)
        W.reserve_workspace(xg, 2, full=True)
        W.dwt_oop_(yg, xg, wt, 2)
        assert W.last_kernel() == "k_fwd2d_tileB"       # (of this stream's context)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        W.dwt_oop_(yg, xg, wt, 2)
    for k in (1, 2, 0):
        xg.copy_(W.to_device(xin[k]))
        yg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(W.to_host(yg), oracle.dwt_filter(xin[k], wt.qmf, 2)), k
    del graph
