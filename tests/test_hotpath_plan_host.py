"""The plan of the hot path's one correlation launch (hotpath.correlation_sets, hotpath.set_bias_table) against literal values worked out by hand
from the loops proto_mask_features had before the plan became a function of its own: no GPU, no device tensor.

A set is (first row, rows) of the proxy table plus the offset of its plane in the flat [O, n_ch, h, w] proto-mask tensor; the cluster sets come
level by level, object by object, (centroid | centroid_avg); the k = 1 sets, one per object, come last."""
import pytest
import torch

from aoc_amd import hotpath as hot


def _layout(mc, n_obj, hw):
    return hot.channel_slices(mc), mc.proto_channels * hw


def test_two_levels():
    mc = hot.MatchingConfig(CLUSTER_LEVELS=[2, 3])
    O, hw = 2, 6
    ch, obj_stride = _layout(mc, O, hw)
    n_ad = hot.adaptive_proxy_rows(mc, O)
    assert (mc.proto_channels, obj_stride, ch["cluster"], ch["proxy"], n_ad) == (26, 156, 1, 5, 24)
    assert hot.proxy_table_rows(mc, O) == 26
    set_begin, set_size, set_off = hot.correlation_sets(mc.cluster_levels, O, hw, obj_stride, ch, n_ad)
    assert set_begin == [0, 3, 6, 9, 12, 15, 18, 21, 24, 25]
    assert set_size == [2, 2, 2, 2, 3, 3, 3, 3, 1, 1]
    assert set_off == [6, 12, 162, 168, 18, 24, 174, 180, 30, 186]


def test_the_banks_layout():
    """IncrementalProxyBank, one level: K = 2, O = 2, capacity 3 frames, R = 2 -- the sets IncrementalProxyBank.handle builds."""
    mc = hot.MatchingConfig(CLUSTER_NUM=2)
    O, hw = 2, 6
    ch, obj_stride = _layout(mc, O, hw)
    assert (mc.proto_channels, obj_stride, ch["cluster"], ch["proxy"]) == (24, 144, 1, 3)
    bank_sets = ([0, 6, 12, 18], [4] * 4, 24)
    set_begin, set_size, set_off = hot.correlation_sets(mc.cluster_levels, O, hw, obj_stride, ch, bank_sets[2], bank_sets)
    assert set_begin == [0, 6, 12, 18, 24, 25]
    assert set_size == [4, 4, 4, 4, 1, 1]
    assert set_off == [6, 12, 150, 156, 18, 162]


def test_the_plan_is_host_lists_of_ints():
    mc = hot.MatchingConfig(CLUSTER_LEVELS=[2, 3])
    ch, obj_stride = _layout(mc, 2, 6)
    for lst in hot.correlation_sets(mc.cluster_levels, 2, 6, obj_stride, ch, 24):
        assert type(lst) is list and all(type(v) is int for v in lst)


def test_the_bias_table():
    a, b = 0.25, -0.5
    bias = torch.tensor([a, b])
    assert hot.set_bias_table(bias, 2).tolist() == [a, a, b, b, a, a, b, b, a, b]
    assert hot.set_bias_table(bias, 1).tolist() == [a, a, b, b, a, b]
    assert hot.set_bias_table(bias, 2).dtype == torch.float32 and hot.set_bias_table(bias, 2).device.type == "cpu"


@pytest.mark.parametrize("levels", [None, [2, 3], [8, 16, 32]])
@pytest.mark.parametrize("radii", [[2, 4], [2, 4, 6, 8, 10, 12]])
@pytest.mark.parametrize("n_obj", [1, 3, 17])
def test_properties(levels, radii, n_obj):
    """Every plane lies inside the tensor, no two sets write the same plane, one bias per set; without the background channels only the object
    stride changes."""
    hw = 63
    plans = {}
    for bg in (True, False):
        mc = hot.MatchingConfig(CLUSTER_LEVELS=levels, MODEL_MULTI_LOCAL_DISTANCE=radii, MODEL_MATCHING_BACKGROUND=bg)
        ch, obj_stride = _layout(mc, n_obj, hw)
        n_ad = hot.adaptive_proxy_rows(mc, n_obj)
        set_begin, set_size, set_off = plans[bg] = hot.correlation_sets(mc.cluster_levels, n_obj, hw, obj_stride, ch, n_ad)
        n_sets = (2 * len(mc.cluster_levels) + 1) * n_obj
        assert len(set_begin) == len(set_size) == len(set_off) == n_sets == hot.set_bias_table(torch.zeros(n_obj), len(mc.cluster_levels)).numel()
        assert all(0 <= off and off + hw <= n_obj * obj_stride and off % hw == 0 for off in set_off)
        assert len(set(set_off)) == n_sets
        assert all(b + s <= hot.proxy_table_rows(mc, n_obj) for b, s in zip(set_begin, set_size))
        plans[bg] = (set_begin, set_size, [(off // obj_stride, off % obj_stride) for off in set_off], obj_stride)
    assert plans[True][:3] == plans[False][:3] and plans[True][3] == plans[False][3] + (1 + len(radii)) * hw
