"""The decoder's memory block without a GPU:

1. decoder_memory.modulate replays the reference's own forward (fixture decoder_memory_rule, five frames with N = 2, 2, 2, 3, 3): the memory
   handed to each modulator and the returned list equal the recording exactly, object identity included where the reference aliases;
2. aoc_cat_film_scale and aoc_groupnorm_relu_scale (and their ops wrappers) reject bad arguments before any launch;
3. a float64 restatement of concat + gate reproduces what the reference's gate 1 returned (fixtures modulator_*), within the bound of a
   float32 nn.Linear of D terms, tanh and one product -- and leaves it with the concatenation reversed."""
import ctypes

import numpy as np
import pytest
import torch

from decoder_memory_bounds import cat_gate_ref, gate1_args
from float64_bounds import U, _check_bound

MODULATOR_GOLDENS = ["modulator_O3", "modulator_O1"]


# ------------------------------------------------------------------------------------------ 1. the memory rule
class Recorder:
    """A decoder object whose two modulators are stand-ins on CPU tensors: they record the memory they are handed and return what the
    reference's Modulator returned on that frame (Modulator_1) or a fresh tensor of the right size (Modulator_2)."""

    def __init__(self, g):
        self.g, self.frame, self.seen = g, 0, {}

    def Modulator_1(self, x, x_memory, IA_head):
        self.seen["x1"], self.seen["m1"] = x, x_memory
        return torch.from_numpy(self.g[f"f{self.frame}_m1_out"])

    def Modulator_2(self, x, x_memory, IA_head):
        self.seen["x2"], self.seen["m2"] = x, x_memory
        return x + 1.0


def test_modulate_replays_the_reference_memory_rule(golden):
    from aoc_amd import decoder_memory
    g = golden("decoder_memory_rule")
    counts = [int(n) for n in g["counts"]]
    assert counts == [2, 2, 2, 3, 3]
    dec = Recorder(g)
    memory = [None, None]
    slot1_objects = []
    for f, N in enumerate(counts):
        dec.frame = f
        x, head = torch.from_numpy(g[f"f{f}_x"]), torch.from_numpy(g[f"f{f}_IA_head"])
        given = list(memory)
        out, new = decoder_memory.modulate(dec, x, head, memory)
        assert all(a is b for a, b in zip(memory, given))                              # the caller's list is left alone
        assert dec.seen["x1"] is x
        assert torch.equal(dec.seen["m1"], torch.from_numpy(g[f"f{f}_m1_memory"])), f"frame {f}: Modulator_1's memory"
        assert torch.equal(dec.seen["m2"], torch.from_numpy(g[f"f{f}_m2_memory"])), f"frame {f}: Modulator_2's memory"
        assert torch.equal(out, torch.from_numpy(g[f"f{f}_m1_out"]) + 1.0)
        assert len(new) == 2
        assert torch.equal(new[0], torch.from_numpy(g[f"f{f}_slot0"])) and torch.equal(new[1], torch.from_numpy(g[f"f{f}_slot1"]))
        # identity: slot 0 is this frame's x by reference (no copy), slot 1 the object that came in unless it was reset
        assert bool(g[f"f{f}_slot0_shares_x"]) and new[0].data_ptr() == x.data_ptr() and not new[0].requires_grad
        assert (new[1] is given[1]) == bool(g[f"f{f}_slot1_is_input_slot1"]), f"frame {f}: slot 1 identity"
        fresh = given[0] is None or given[0].size() != x.size()
        assert (dec.seen["m1"].data_ptr() == x.data_ptr()) == fresh                    # first frame / new object count: x with itself
        slot1_objects.append(new[1])
        memory = new
    assert [bool(g[f"f{f}_slot1_is_input_slot1"]) for f in range(5)] == [False, True, True, False, True]
    assert slot1_objects[0] is slot1_objects[1] is slot1_objects[2]                     # sticky: still frame 0's Modulator_1 output
    assert torch.equal(slot1_objects[2], torch.from_numpy(g["f0_m1_out"]))
    assert not torch.equal(slot1_objects[2], torch.from_numpy(g["f2_m1_out"]))          # ... and not the previous frame's
    assert slot1_objects[3] is slot1_objects[4] and torch.equal(slot1_objects[4], torch.from_numpy(g["f3_m1_out"]))


def test_select_memory():
    from aoc_amd import decoder_memory
    select_memory = decoder_memory.select_memory
    a, b, c = torch.zeros(2, 3, 4, 5), torch.ones(2, 3, 4, 5), torch.ones(3, 3, 4, 5)
    assert select_memory(a, None) is a and select_memory(a, b) is b and select_memory(a, c) is a
    assert select_memory(a, torch.ones(2, 3, 5, 4)) is a


# ------------------------------------------------------------------------------------------ 2. argument validation
@pytest.fixture(scope="module")
def L():
    try:
        import aoc_amd
        return aoc_amd._lib.lib()
    except (OSError, ImportError, RuntimeError) as e:
        pytest.skip(f"the HIP library cannot be loaded here: {e}")


def test_entry_points_reject_bad_arguments_before_any_launch(L):
    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    cat = lambda x=p, mem=p, head=p, w=p, b=p, n=2, D=5, Cx=3, Cm=3, hw=7, y=p: L.aoc_cat_film_scale(x, mem, head, w, b, n, D, Cx, Cm, hw, y, None)
    assert cat(x=None) == INVALID and cat(mem=None) == INVALID and cat(head=None) == INVALID and cat(w=None) == INVALID and cat(y=None) == INVALID
    assert cat(n=0) == INVALID and cat(n=-1) == INVALID and cat(D=0) == INVALID and cat(Cx=0) == INVALID and cat(Cm=-1) == INVALID
    assert cat(hw=0) == INVALID and cat(hw=-7) == INVALID
    assert cat(n=300, Cx=200, Cm=100) == UNSUPPORTED                                # more planes than one grid dimension holds
    need = L.aoc_groupnorm_relu_workspace_bytes(2, 4)
    gn = lambda x=p, N=2, C=8, hw=7, groups=4, res=p, head=p, w=p, gb=p, D=5, y=p, ws=p, nbytes=need: L.aoc_groupnorm_relu_scale(
        x, N, C, hw, groups, p, p, 1e-5, res, 1, head, w, gb, D, y, ws, nbytes, None)
    assert gn(x=None) == INVALID and gn(head=None) == INVALID and gn(w=None) == INVALID and gn(y=None) == INVALID and gn(ws=None) == INVALID
    assert gn(N=0) == INVALID and gn(C=0) == INVALID and gn(hw=-1) == INVALID and gn(groups=0) == INVALID and gn(D=0) == INVALID
    assert gn(C=8, groups=3) == INVALID                                             # C not divisible by groups
    assert gn(N=300, C=256, groups=4) == UNSUPPORTED
    assert gn(nbytes=need - 1) == WORKSPACE


def test_wrappers_reject_mismatched_shapes_without_a_device():
    """Cx + Cm against the weight's rows is not expressible in the C signature (it has no row count): the wrapper checks it, before it
    asks for a device."""
    from aoc_amd import ops
    x, mem, head = torch.zeros(2, 3, 4, 5), torch.zeros(2, 5, 4, 5), torch.zeros(2, 6)
    with pytest.raises(ValueError):
        ops.cat_film_scale(x, mem, head, torch.zeros(7, 6), torch.zeros(7))          # 3 + 5 channels, 7 rows
    with pytest.raises(ValueError):
        ops.cat_film_scale(x, mem, head, torch.zeros(8, 6), torch.zeros(7))
    with pytest.raises(ValueError):
        ops.cat_film_scale(x, mem, head, torch.zeros(8, 5), None)                   # head dimension
    with pytest.raises(ValueError):
        ops.cat_film_scale(x, torch.zeros(2, 5, 5, 4), head, torch.zeros(8, 6), None)
    with pytest.raises(ValueError):
        ops.cat_film_scale(x, None, head, torch.zeros(8, 6), None)                  # Cm = 0: three rows wanted
    with pytest.raises(ValueError):
        ops.groupnorm_relu_scale(torch.zeros(2, 8, 7), 3, None, None, 1e-5, None, True, head, torch.zeros(8, 6), None)
    with pytest.raises(ValueError):
        ops.groupnorm_relu_scale(torch.zeros(2, 8, 7), 4, None, None, 1e-5, None, True, head, torch.zeros(9, 6), None)
    from aoc_amd import _lib
    with pytest.raises(_lib.AocHipError):                                                # well-formed, but on the CPU: no fallback
        ops.cat_film_scale(x, mem, head, torch.zeros(8, 6), torch.zeros(8))


# ------------------------------------------------------------------------------------------ 3. fixture self-check
@pytest.mark.parametrize("name", MODULATOR_GOLDENS)
def test_reference_reproduces_the_golden_gate_1(name, golden):
    g = golden(name)
    args = gate1_args(g)
    assert np.array_equal(g["gate1_in"], np.concatenate([g["in_x"], g["in_x_memory"]], 1))          # :193, exact
    want, tol = cat_gate_ref(*args)
    _check_bound(torch.from_numpy(g["gate1_out"]), want, tol, cat_gate_ref(*args, reverse=True)[0], f"{name}: gate 1, concat reversed")
    assert float(tol.max()) < 64 * U * float(want.abs().max())                                       # of the size of float32 roundings
    assert g["out_f32"].shape == g["out_f64"].shape == (args[0].shape[0], args[0].shape[1]) + args[0].shape[2:]
