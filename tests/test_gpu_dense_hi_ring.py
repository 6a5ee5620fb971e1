"""The dense kernel with hi planes only in its LDS ring (eight tiles per step, lo planes of rescored tiles from global memory) computes, bit for
bit, what the kernel with whole records in the ring computed: tests/golden/dense_hi_ring_parent.json holds the SHA-256 of the op's fp32
output on the commit before the change, written by tools/record_dense_hashes.py (which also defines the cases).  A pair's exact value does
not depend on what else was evaluated and the change keeps every pair's operation order, so equality is exact, not within a tolerance.

The cases: cfg2 size with the bench's pools at 1 / 6 / 12 frames, nine objects, pools whose tile count per split is below one chunk of eight,
exactly one, one more and every residue mod 8, absent objects, an object of fewer than 32 rows, a pool that is not whole frames, the ties /
duplicates / mixed-norm pool, the query frame inside the pool."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ATOL = 5e-6          # on proto-mask outputs: the tolerance of test_gpu_dense_split.py::test_split_matches_fp32_and_oracle

_spec = importlib.util.spec_from_file_location(
    "record_dense_hashes", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "record_dense_hashes.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def aoc():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()
    return aoc_amd


@pytest.fixture(scope="module")
def fixture_hashes():
    with open(rec.FIXTURE) as f:
        return json.load(f)


def test_fixture_lists_exactly_the_cases(fixture_hashes):
    assert sorted(fixture_hashes) == sorted(rec.CASES)


@pytest.mark.parametrize("name", list(rec.CASES))
def test_output_hash_equals_the_parent_commits(aoc, fixture_hashes, name):
    q, pool, lab = rec.CASES[name]()
    for _ in range(2):                                    # the set of rescored tiles depends on timing; the result must not
        out, st = rec.run_case(aoc.ops, q, pool, lab)
        print(name, "tested", st["tested"], "rescored", st["rescored"], "tiles", st["tiles"])
        # the split path ran (a take-over by the exact-fp32 kernels leaves the counters at zero); the counts themselves are development aids
        assert st["tested"] > 0
        if name not in rec.DEGENERATE:
            assert st["rescored"] > 0
        assert rec.digest(out) == fixture_hashes[name]


@pytest.mark.parametrize("name", rec.SMALL)
def test_small_cases_against_the_oracle(aoc, name):
    """Independent of the fixture: the cases the CPU oracle can afford, transformed output, at the tolerance the existing split test uses."""
    from oracle import matching as om
    q, pool, lab = rec.CASES[name]()
    assert q.shape[0] * pool.shape[0] <= rec.ORACLE_LIMIT
    o = lab.shape[1]
    bias = torch.linspace(-0.3, 0.3, o)
    got, st = rec.run_case(aoc.ops, q, pool, lab, bias=bias, transform=True)
    assert st["tested"] > 0
    qt, pt, lt = torch.from_numpy(q), torch.from_numpy(pool), torch.from_numpy(lab)
    want = om.proto_transform(om.nearest_neighbor_features_per_object(pt, qt, lt).squeeze(-1), bias.view(1, -1))
    np.testing.assert_allclose(got.t().numpy(), want.numpy(), rtol=0, atol=ATOL)
