"""modwt_batch / imodwt_batch in the opt-in fused arithmetic mode (libwavelets_mi355x_fma.so): one case per tier against the
tolerance contract tests/test_gpu_fused.py applies to modwt (reference = the Float64 oracle on the same inputs).  Bit equality
between the tiers is not claimed in this mode."""
import numpy as np
import pytest

import modwt_batch_cases as MC
from test_gpu_fused import _check, fused  # noqa: F401  (the fixture switches the library and switches back)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_fused_modwt_batch_on_both_tiers(fused, oracle, dtype):
    W = fused
    import torch
    wt = W.wavelet(W.WT.db4)
    L = 6
    for n, B, kernels in ((1000, 4, ("k_modwt_lds", "k_imodwt_lds")), (1 << 14, 3, ("k_modwt_step_b", "k_imodwt_step_b"))):
        us = MC.units(n, B, dtype)
        y = W.modwt_batch(W.to_device(np.ascontiguousarray(us.T)), wt, L)
        kf = W.last_kernel()
        xr = W.imodwt_batch(y, wt)
        ki = W.last_kernel()
        torch.cuda.synchronize()
        assert (kf, ki) == kernels, (n, kf, ki)
        yh, xh = W.to_host(y), W.to_host(xr)
        for u in range(B):
            ref = oracle.modwt(us[u].astype(np.float64), wt.qmf, L)
            _check(yh[:, :, u], ref, L, dtype == np.float64)
            _check(xh[:, u], oracle.imodwt(ref, wt.qmf), L, dtype == np.float64)
