"""modwt_mra_batch in the opt-in fused arithmetic mode (libwavelets_mi355x_fma.so): one case per tier against the tolerance contract
tests/test_gpu_fused.py applies to modwt (reference = the Float64 oracle loop -- imodwt of the coefficient matrix with every column
but one set to zero -- on the same coefficients).  Bit equality between the tiers is not claimed in this mode."""
import numpy as np
import pytest

import modwt_mra_cases as RC
from test_gpu_fused import _check, fused  # noqa: F401  (the fixture switches the library and switches back)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_fused_modwt_mra_batch_on_both_tiers(fused, oracle, dtype):
    W = fused
    import torch
    wt = W.wavelet(W.WT.db4)
    L = 6
    for n, B, kernel in ((1000, 4, "k_modwt_mra_lds"), (1 << 14, 3, "k_modwt_mra_step_b")):
        co = RC.forward(oracle, W, "db4", n, B, dtype, L)                    # (B, L + 1, n), the exact coefficients in the element type
        y = W.modwt_mra_batch(W.to_device(np.ascontiguousarray(co.transpose(2, 1, 0))), wt)
        assert W.last_kernel() == kernel, (n, W.last_kernel())
        torch.cuda.synchronize()
        yh = W.to_host(y)
        for u in range(B):
            ref = RC.mra_of(oracle, wt.qmf, co[u].astype(np.float64))
            _check(yh[:, :, u], ref.T, L, dtype == np.float64)
