"""Every kernel instance the library ships against the oracle (tests/instance_cases.py: one block of rows per kernel family, generated
over what selects the template arguments -- element type, tap count or scheme shape, and the launchers' options for what they pick by
size).

Per family: every row forward on rng_array normals and inverse on the oracle's forward output, W.last_kernel() is the kernel the row
names, and the results equal the oracle's bit for bit (np.array_equal); the threshold, selection and denoise rows bit for bit against
oracle.threshold / mad / denoise; the k_entropy_seg rows against tests/bestbasis_ref.py under the bounds of DESIGN.md section 11 that
the module states.  A row that reports another kernel than it names is a failure of the table.

Which instances these rows launch is not restated here: tools/instance_trace.py measures it (tests/instances_reached.json), and
test_instance_coverage.py holds the library's symbols to that record.
"""
import pytest

import instance_cases as IC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", list(IC.FAMILIES))
def test_every_row_of_the_family(gpu, W, oracle, family):
    bad = []
    for row in IC.FAMILIES[family]:
        bad += IC.run_row(W, oracle, row)
    assert not bad, bad
