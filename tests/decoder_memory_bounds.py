"""References and bounds shared by test_decoder_memory_host.py and test_gpu_decoder_memory.py (conventions of float64_bounds.py: U, gamma, and
4 U for tanhf with the addition of 1).  No constant here is fitted to output."""
import torch

from float64_bounds import U, gamma, t64


def cat_gate_ref(x, mem, head, weight, bias, reverse=False):
    """float64 concat + gate with the bound for a float32 evaluation: a Linear of D terms in any order (gamma(D + 1) on sum |h w| + |b|),
    tanh' <= 1, tanhf and the addition of 1 within 4 U (float64_bounds), one rounding for the product with x."""
    D = head.shape[1]
    cat = torch.cat([mem, x], 1) if reverse else torch.cat([x, mem], 1)
    gain = 1.0 + torch.tanh(head @ weight.t() + bias)
    dgain = gamma(D + 1) * (head.abs() @ weight.abs().t() + bias.abs()) + 4 * U
    want = gain[:, :, None, None] * cat
    spread = cat.abs() * dgain[:, :, None, None]
    return want, spread + U * (want.abs() + spread)


def gate1_args(g):
    return (t64(g["in_x"]), t64(g["in_x_memory"]), t64(g["in_IA_head"]), t64(g["p_M1_Reweight_Layer_1.IA.weight"]),
            t64(g["p_M1_Reweight_Layer_1.IA.bias"]))


def gate_chain_ref(x, head, gates, widths, dx=None):
    """x through gate, channel slice, gate, slice, ... in float64 (what a modulator is with channel-slicing stand-ins for its Bottlenecks):
    gates = [(weight, bias), ...], widths = the channels kept after each gate.  The value is x times a product of gains; its bound follows
    from the gains' bounds (cat_gate_ref) multiplied out, not linearised, and one rounding per product; dx is what x itself is already off
    by (the chain is linear in x)."""
    D = head.shape[1]
    C = x.shape[1]
    prod = torch.ones(x.shape[0], C, dtype=torch.float64)
    hi = torch.ones_like(prod)
    for (weight, bias), keep in zip(gates, widths):
        gain = 1.0 + torch.tanh(head @ weight.t() + bias)
        dgain = gamma(D + 1) * (head.abs() @ weight.abs().t() + bias.abs()) + 4 * U
        prod, hi = (prod[:, :gain.shape[1]] * gain)[:, :keep], (hi[:, :gain.shape[1]] * (gain + dgain))[:, :keep]
    n = len(gates)
    keep = prod.shape[1]
    xs = x[:, :keep]
    want = prod[:, :, None, None] * xs
    dxs = torch.zeros_like(xs) if dx is None else dx[:, :keep]
    return want, (xs.abs() + dxs) * ((hi - prod) + gamma(n) * hi)[:, :, None, None] + dxs * prod[:, :, None, None]
