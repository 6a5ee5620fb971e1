"""hotpath.proto_mask_features in the orchestration modes the one-call C path (FrameRunner / aoc_frame_enqueue) is no oracle for -- the inline
chain with `rng`, a carried dense_state, cluster_state with a side stream, a batched chain of two frames, dense_stream, deferred correlations of two
sequences, dense_precision="fp32", the incremental bank, float16 matching with and without a handle, match_pool at an atrous rate, two levels,
17 objects, another width -- computes, bit for bit, what its one-body version computed: tests/golden/hotpath_modes_parent.json holds the SHA-256
of the proto-mask tensor and of the attention head for every frame of every case on the commit before the function was cut into stages,
written by tools/record_hotpath_modes.py (which also defines the cases).  The stages enqueue the same calls in the same order on the same
streams, so equality is exact."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "record_hotpath_modes", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "record_hotpath_modes.py"))
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
def fixture_cases():
    with open(rec.FIXTURE) as f:
        return json.load(f)["cases"]


def test_fixture_lists_exactly_the_cases(aoc, fixture_cases):
    assert sorted(fixture_cases) == sorted(rec.CASES)
    for name, case in rec.CASES.items():
        assert fixture_cases[name]["size"] == list(case["size"]) and fixture_cases[name]["seed"] == case["seed"]
        assert rec.meets_condition(aoc.synthetic, case), f"{name}: an object of the first pool frame has fewer than kmax labelled pixels"


@pytest.mark.parametrize("name", list(rec.CASES))
def test_hashes_equal_the_parent_commits(aoc, fixture_cases, name):
    got, want = rec.digests(rec.run_case(aoc, name)), fixture_cases[name]["frames"]
    assert len(got) == len(want) == rec.FRAMES * (2 if "seed_b" in rec.CASES[name] else 1)
    for t, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: result {t} differs from the parent commit's ({'feat' if g['feat'] != w['feat'] else 'head'})"
