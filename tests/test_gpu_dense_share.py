"""dense_prune_kernel as resident workgroups that walk the work list, on the MI355X: the same bits at every CU budget and dense share.

The shapes are the budget cases of carried_state_cases.py (m = 150, 513, 1100: one to three query blocks, 150 not a multiple of 32; a pool
of 3 tiles and one of more than 64; a build and one plan-reusing call; raw and transformed).  The run at the whole share and budget 0 is
held to the float64 bound by test_gpu_carried_state.run_sequence; every run of test_dense_share_host.GPU_COMBOS is array_equal to it.
test_dense_share_host.py shows without a GPU that those combinations reach one workgroup that walks everything, a grid that leaves a
remainder, a grid as large as the list and lists of fewer than 8 items."""
import numpy as np
import pytest
import torch

import carried_state_cases as cs
import test_gpu_carried_state as tcs
from test_dense_share_host import GPU_COMBOS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aoc():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()      # raises if the HIP library is missing: no silent fallback
    return aoc_amd


@pytest.fixture(autouse=True)
def default_share(aoc):
    """Whatever a test sets, the share and the budget the process started with are in force again afterwards."""
    before = aoc._lib.lib().aoc_dense_share()
    yield
    aoc.ops.set_stream_cus(0, dense_share=before)


@pytest.mark.parametrize("pool", list(cs.BUDGET_POOLS))
@pytest.mark.parametrize("m", cs.BUDGET_M)
def test_share_and_budget_change_no_bit(aoc, m, pool):
    seq = cs.budget_case(m, pool).name
    base = {}
    aoc.ops.set_stream_cus(0, dense_share=256)
    for transform in (False, True):
        base[transform] = tcs.run_sequence(aoc, seq, True, transform)                 # held to the float64 bound
    for budget, share in GPU_COMBOS:
        aoc.ops.set_stream_cus(budget, dense_share=share)
        for transform in (False, True):
            outs = tcs.run_sequence(aoc, seq, True, transform, check=False)
            assert len(outs) == len(base[transform]) == 2
            for k, (a, b) in enumerate(zip(outs, base[transform])):
                assert np.array_equal(a, b), (f"{seq} budget {budget} share {share}/256 step {k} transform={transform}: "
                                              f"{int((a != b).sum())} outputs differ from budget 0 at the whole share")
