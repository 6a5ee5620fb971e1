"""Drop-in mirrors of the memory block of ``CalibrationDecoding`` (networks/aoc/decoding_module.py) on the HIP library: ``Modulator_1`` and
``Modulator_2`` (192-210) and ``modulate``, the lines 133-140 and 148 of ``forward`` that choose, use and hand back the two memories.  They are
functions of the decoder object, so they bind onto the reference's class or run on any object that carries the attributes
they read.  The convolutions stay PyTorch modules (MIOpen); the concatenation, the gates and the normalisations run in libaoc_hip.so, and the
memories never leave the device."""
from . import gct, ops


def _gate_args(gate):
    ia = gate.IA                                                       # ATT:10, the reference's parameter name
    return ia.weight.detach(), ia.bias.detach() if ia.bias is not None else None


def _modulator(dec, prefix, x, x_memory, IA_head):
    gates = [getattr(dec, f"{prefix}_Reweight_Layer_{i}") for i in (1, 2, 3)]
    blocks = [getattr(dec, f"{prefix}_Bottleneck_{i}") for i in (1, 2, 3)]
    ops.inference_only(prefix, x, x_memory, IA_head, *(g.IA.weight for g in gates))
    # :193-194 / :203-204 in one launch: the concatenation is never written ungated
    x = ops.cat_film_scale(x, x_memory, IA_head, *_gate_args(gates[0]))
    for i, block in enumerate(blocks):
        following = gates[i + 1] if i + 1 < 3 else None
        if following is None:
            x = block(x)                                               # :199 / :209
        elif isinstance(block, gct.Bottleneck):
            x = block(x, gate=(IA_head,) + _gate_args(following))      # :195-196, :197-198: the gate rides on bn3's apply pass
        else:
            x = ops.film_scale(block(x), IA_head, *_gate_args(following))
    return x


def Modulator_1(dec, x, x_memory, IA_head):
    """decoding_module.py:192-200.  Reads dec.M1_Reweight_Layer_{1,2,3} and dec.M1_Bottleneck_{1,2,3}."""
    return _modulator(dec, "M1", x, x_memory, IA_head)


def Modulator_2(dec, x, x_memory, IA_head):
    """decoding_module.py:202-210.  Reads dec.M2_Reweight_Layer_{1,2,3} and dec.M2_Bottleneck_{1,2,3}."""
    return _modulator(dec, "M2", x, x_memory, IA_head)


def select_memory(current, slot):
    """decoding_module.py:134-135 / :138-139: a slot that is None, or whose size differs from the current tensor's (the object count changed),
    takes the current tensor; any other slot is used as it is."""
    if slot is None or current.size() != slot.size():
        return current
    return slot


def modulate(dec, x, IA_head, memory_list):
    """decoding_module.py:133-140 and :148 as one call: x is the ASPP output (:131); -> (x after both modulators, the next frame's memory_list).

    The reference's rule, exactly: on a sequence's first frame and whenever the object count changes a modulator sees its input concatenated
    with itself; slot 0 is returned as THIS frame's ASPP output; slot 1 is returned unchanged, so it stays the first Modulator_1 output of its
    size for the rest of the sequence (it is never refreshed).  Both stay on x's device and nothing is copied: ``x.detach()`` is held by
    reference, where the reference moves both memories to the host and back on every frame (``.cpu()`` :148, ``.cuda()`` :136, :140).

    Precondition: the caller's ASPP output must not be a buffer that the next frame overwrites before that frame's modulators have run (slot 0
    aliases it).  memory_list itself is not modified.  A reference ``forward`` that still calls ``.cuda()`` / ``.cpu()`` on these tensors
    keeps working: both are the identity or a plain copy of a device tensor."""
    cur_1 = x.detach()                                                 # :133
    mem_1 = select_memory(cur_1, memory_list[0])                       # :134-135
    x = dec.Modulator_1(x, mem_1, IA_head)                             # :136
    cur_2 = x.detach()                                                 # :137
    mem_2 = select_memory(cur_2, memory_list[1])                       # :138-139
    x = dec.Modulator_2(x, mem_2, IA_head)                             # :140
    return x, [cur_1, mem_2]                                           # :148
