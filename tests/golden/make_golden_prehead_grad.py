#!/usr/bin/env python3
"""Golden vectors for the differentiable DynamicPreHead (tests/test_prehead_grad_host.py, tests/test_gpu_prehead_grad.py), recorded by running
the reference's OWN ``DynamicPreHead`` (networks/aoc/decoding_module.py:228-240) UNMODIFIED on the CPU, in float64, under autograd, followed
by the concatenation of aocnet.py:362 written out (``torch.cat((emb.expand(O, -1, -1, -1), pre_to_cat), 1)``, aocnet.py:188 for the
expansion), with the loss ``(out * weight).sum()`` for a fixed random ``weight``.  None of the reference's text is stored, and nothing is
written into its tree.

Recorded per case (prehead_grad_*.npz): the float16-representable inputs (``in_x`` [O, n_in, h, w], ``in_emb`` [C, h, w] or absent,
``in_weight``), the four parameters (float16-representable), the loss and the float64 gradients of x, the embedding and the parameters -- no
activation.  A fixture must not sit near the ReLU's corner: the recorder refuses a case with an undecided element
(prehead_grad_bounds.prehead_grad_ref).  The files are written with a fixed time stamp, so a second run reproduces them byte for byte.

    python tests/golden/make_golden_prehead_grad.py <the reference's complete_project/AOCNet directory>
    python tests/golden/make_golden_prehead_grad.py --seeds          # the seeds of prehead_grad_bounds' cases (needs no reference)
"""
import io
import os
import sys
import warnings
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True                            # never write into the reference tree
import prehead_grad_bounds as pgb  # noqa: E402
warnings.simplefilter("ignore")
torch.set_num_threads(4)
f64 = np.float64


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def save(path, arrays):
    """np.savez_compressed with a fixed time stamp: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def case(dm, name, seed, O, n_in, n_out, h, w, C):
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    n = rs.standard_normal
    pre = dm.DynamicPreHead(in_dim=n_in, embed_dim=n_out)                     # the reference's class, unmodified
    params = dict(conv_w=h16(n((n_out, n_in, 1, 1)) * np.sqrt(2.0 / n_in)), conv_b=h16(0.2 * n(n_out)), gn_w=h16(1.0 + 0.25 * n(n_out)), gn_b=h16(0.5 * n(n_out)))
    with torch.no_grad():
        for p, a in zip((pre.conv.weight, pre.conv.bias, pre.bn.weight, pre.bn.bias), params.values()):
            p.copy_(torch.from_numpy(a.astype(f64)))
    x, weight = h16(n((O, n_in, h, w))), h16(n((O, C + n_out, h, w)))
    emb = h16(n((C, h, w))) if C else None
    lx = torch.from_numpy(x.astype(f64)).requires_grad_(True)
    le = torch.from_numpy(emb.astype(f64)).requires_grad_(True) if C else None
    out = pre(lx)                                                            # aocnet.py:360
    if C:
        out = torch.cat((le.unsqueeze(0).expand(O, -1, -1, -1), out), 1)     # aocnet.py:188, 362
    loss = (out * torch.from_numpy(weight.astype(f64))).sum()
    loss.backward()
    _, und = pgb.prehead_grad_ref(weight.reshape(O, C + n_out, -1), x.reshape(O, n_in, -1), params["conv_w"], params["conv_b"], pre.bn.num_groups,
                                  params["gn_w"], params["gn_b"], pre.bn.eps, C)
    assert int(und.sum()) == 0, f"{name}: {int(und.sum())} elements near the ReLU's corner; take another seed"
    arrays = dict(in_x=x, in_weight=weight, seed=np.int64(seed), groups=np.int64(pre.bn.num_groups), eps=np.float64(pre.bn.eps), loss=np.float64(loss.item()),
                  grad_x=lx.grad.numpy(), grad_conv_w=pre.conv.weight.grad.numpy(), grad_conv_b=pre.conv.bias.grad.numpy(),
                  grad_gn_w=pre.bn.weight.grad.numpy(), grad_gn_b=pre.bn.bias.grad.numpy(), **{"w_" + k: v for k, v in params.items()})
    if C:
        arrays.update(in_emb=emb, grad_emb=le.grad.numpy())
    path = os.path.join(HERE, name + ".npz")
    save(path, arrays)
    size = os.path.getsize(path)
    assert size < 100_000, f"{name}: {size} bytes"
    print(f"{name}: {size} bytes, loss {loss.item():.6f}, active share {float((out[:, C:] > 0).double().mean()):.3f}")


def seeds():
    for label, cases, build in (("CASES", pgb.CASES, pgb.case), ("MASK_CASES", pgb.MASK_CASES, pgb.case), ("PLANTED", {pgb.PLANTED: 0}, pgb.planted_case)):
        print(label, {k: pgb.first_seed(k, build) for k in cases})


def main(ref_root):
    from make_golden_decoder_tail import load_reference
    dm = load_reference(ref_root)[2]
    case(dm, pgb.FIXTURES[0], 701, 1, 24, 64, 9, 11, 0)
    case(dm, pgb.FIXTURES[1], 702, 3, 26, 64, 7, 9, 5)
    case(dm, pgb.FIXTURES[2], 703, 4, 24, 64, 5, 5, 100)


if __name__ == "__main__":
    if sys.argv[1] == "--seeds":
        seeds()
    else:
        main(os.path.abspath(sys.argv[1]))
