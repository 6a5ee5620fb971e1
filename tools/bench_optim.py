"""Developer tool (GPU box): one training update -- gradient-norm clip, Nesterov SGD, zeroing of the gradients -- in arms that alternate step by
step in one process:
  (ref)    the reference's construction (train_manager_mm.py:68-72, 283-284; utils/learning.py:24-34): one group per parameter,
           torch.nn.utils.clip_grad_norm_ + torch.optim.SGD(momentum=0.9, nesterov=True).step() + zero_grad(set_to_none=False);
  (hip)    aoc_amd.optim_train.SGD(clip_grad_norm=5.0).step(zero_grads=True) over the same groups (csrc/optim.hip behind it);
  (single) for information: torch with all parameters in a single group;
  (fused)  for information: the single group with fused=True, where this torch build accepts it for SGD.
Two parameter lists: the decoder and DynamicPreHead shapes recorded in tests/golden/integration_decoder.json plus the embedding head of
aocnet.py:19-28; and the same with a ResNet-101-shaped backbone in front, whose shapes are generated here from the layer plan [3, 4, 23, 3].
Per arm: WARMUP steps, then RUNS steps each bracketed by two device events (median / min / max: the step as the stream sees it, host gaps
included); host_enqueue = the host time of the step's calls after a synchronisation, without waiting for the device; launches = the device events of torch's profiler over one step, the
optimiser's own annotation left out (for the hip arm also from the code: sums, finish, step); the bytes the arm's composition moves (ref: fifteen
parameter-sized streams, hip: seven -- g twice, p and the buffer read and written, g zeroed) over the median, against the measured copy peak
of 6.29 TB/s.  Before every step the gradients are refilled, outside the timed region.  Then the hip arm's three entries alone, to see whether
the update pass finds the gradients in the last-level cache.  The merge condition: the hip arm's median is below the ref arm's on both lists
(exit status 1 otherwise, or when the arms' parameters drift apart).

    python tools/bench_optim.py [out.txt]        # default: profiles/optim_ab.txt
"""
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import aoc_amd  # noqa: E402
from aoc_amd import optim_train as ot  # noqa: E402

WARMUP, RUNS = 5, 20
LR, MAX_NORM, WD = 0.01, 5.0, 1e-4
COPY_PEAK = 6.29e12
STREAMS = {"ref": 15, "hip": 7, "single": 15, "fused": 7}
# the arms round differently (torch fuses a + alpha * b in some paths); after a few steps from equal parameters they agree to a few float32 ulps
DRIFT_TOL = 1e-5


def decoder_shapes():
    with open(os.path.join(ROOT, "tests", "golden", "integration_decoder.json")) as f:
        sd = json.load(f)["state_dict"]
    out = [("decoder." + k, v) for k, v in sd["decoder"].items()] + [("dynamic_prehead." + k, v) for k, v in sd["DynamicPreHead"].items()]
    emb, aspp = 100, 256                                   # aocnet.py:19-28: depthwise 3x3 + GroupNorm, 1x1 to the embedding + GroupNorm, the two biases
    out += [("seperate_conv.weight", [aspp, 1, 3, 3]), ("seperate_conv.bias", [aspp]), ("bn1.weight", [aspp]), ("bn1.bias", [aspp]),
            ("embedding_conv.weight", [emb, aspp, 1, 1]), ("embedding_conv.bias", [emb]), ("bn2.weight", [emb]), ("bn2.bias", [emb]),
            ("bg_bias", [1, 1, 1, 1]), ("fg_bias", [1, 1, 1, 1])]
    return out


def resnet101_shapes(plan=(3, 4, 23, 3)):
    """bottleneck ResNet: a 7x7 stem, then per stage `plan[i]` blocks of 1x1, 3x3, 1x1 (expansion 4) with a norm each, a projection in the first"""
    out = [("backbone.conv1.weight", [64, 3, 7, 7]), ("backbone.bn1.weight", [64]), ("backbone.bn1.bias", [64])]
    inplanes = 64
    for stage, (blocks, planes) in enumerate(zip(plan, (64, 128, 256, 512)), 1):
        for b in range(blocks):
            name = f"backbone.layer{stage}.{b}."
            for k, shape in enumerate(([planes, inplanes, 1, 1], [planes, planes, 3, 3], [planes * 4, planes, 1, 1]), 1):
                out += [(f"{name}conv{k}.weight", shape), (f"{name}bn{k}.weight", [shape[0]]), (f"{name}bn{k}.bias", [shape[0]])]
            if b == 0:
                out += [(name + "downsample.0.weight", [planes * 4, inplanes, 1, 1]), (name + "downsample.1.weight", [planes * 4]),
                        (name + "downsample.1.bias", [planes * 4])]
            inplanes = planes * 4
    return out


class Arm:
    def __init__(self, kind, shapes, src_params, src_grads):
        self.kind = kind
        self.params = [torch.nn.Parameter(p.clone()) for p in src_params]
        self.src = src_grads
        for p, g in zip(self.params, src_grads):
            p.grad = g.clone()
        groups = [{"params": [p], "lr": LR, "weight_decay": 0.0 if "beta" in name else WD} for (name, _), p in zip(shapes, self.params)]
        if kind == "hip":
            self.opt = ot.SGD(groups, lr=LR, momentum=0.9, nesterov=True, clip_grad_norm=MAX_NORM)
        elif kind == "ref":
            self.opt = torch.optim.SGD(groups, lr=LR, momentum=0.9, nesterov=True)
        else:
            self.opt = torch.optim.SGD(self.params, lr=LR, momentum=0.9, nesterov=True, weight_decay=WD, **({"fused": True} if kind == "fused" else {}))

    def refill(self):
        torch._foreach_copy_([p.grad for p in self.params], self.src)

    def step(self):
        if self.kind == "hip":
            self.opt.step(zero_grads=True)
        else:
            torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
            self.opt.step()
            self.opt.zero_grad(set_to_none=False)


def count_launches(arm):
    try:
        from torch.profiler import ProfilerActivity, profile
        arm.refill()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            arm.step()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and not e.name.startswith(("Optimizer.", "ProfilerStep"))]
        if not names:
            return "n/a"
        short = [(re.findall(r"(\w+)(?:<[^()]*>)?\(", n) or [n[:40]])[0] for n in names]            # the kernel's own name out of its signature
        return str(len(names)) + (" [" + ", ".join(short) + "]" if len(names) <= 6 else "")
    except Exception as e:                                 # the profiler is a convenience here, the count from the code stands without it
        return f"n/a ({type(e).__name__})"


def event_ms(call, before=None):
    if before:
        before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_list(title, shapes, gen, lines):
    n = sum(int(np.prod(s)) for _, s in shapes)
    src_p = [torch.randn(*s, device="cuda", generator=gen) for _, s in shapes]
    src_g = [torch.randn(*s, device="cuda", generator=gen) * 0.01 for _, s in shapes]
    kinds = ["ref", "hip", "single"]
    arms = {}
    for kind in kinds + ["fused"]:
        try:
            arms[kind] = Arm(kind, shapes, src_p, src_g)
        except (RuntimeError, ValueError, TypeError) as e:
            lines.append(f"#   ({kind}) not available in this torch build: {str(e).splitlines()[0][:120]}")
    order = [k for k in ("ref", "hip", "single", "fused") if k in arms]
    for _ in range(WARMUP):
        for k in order:
            arms[k].refill()
            arms[k].step()
    torch.cuda.synchronize()
    drift = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(arms["hip"].params, arms["ref"].params))
    ms = {k: [] for k in order}
    host = {k: [] for k in order}
    for _ in range(RUNS):
        for k in order:
            ms[k].append(event_ms(arms[k].step, arms[k].refill))
        for k in order:
            arms[k].refill()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arms[k].step()
            host[k].append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
    lines.append(f"{title}: {len(shapes)} tensors, {n / 1e6:.2f} M parameters ({n * 4 / 1e6:.1f} MB per parameter-sized stream); hip table uploads "
                 f"{arms['hip'].opt.table_uploads}; max |hip - ref| / max |ref| after {WARMUP} steps {drift:.1e}")
    med = {}
    for k in order:
        med[k] = float(np.median(ms[k]))
        moved = STREAMS[k] * n * 4
        launches = count_launches(arms[k]) + (" (from the code: 3)" if k == "hip" else "")
        lines.append(f"  ({k:6s}) device {med[k]:8.3f} ms [{min(ms[k]):.3f}, {max(ms[k]):.3f}]   host_enqueue {np.median(host[k]):8.3f} ms   launches {launches}   "
                     f"{STREAMS[k]} streams = {moved / 1e6:.1f} MB -> {moved / med[k] / 1e9:.2f} TB/s ({100 * moved / (med[k] * 1e-3) / COPY_PEAK:.0f} % of the copy peak)")
    # the three entries alone, on the hip arm's own table
    hip = arms["hip"]
    table, L = hip.opt._table, aoc_amd._lib.lib()
    partial = torch.empty(max(table.n_chunks, 1), dtype=torch.float64, device="cuda")
    norm, coef = torch.empty(1, device="cuda"), torch.ones(1, device="cuda")
    rows = (("sums (g once)", lambda: ot.grad_sumsq_partials(table, partial), 1), ("finish", lambda: ot.grad_norm_finish(partial, table.n_chunks, MAX_NORM, norm, coef), 0),
            ("step (g, p, b in; p, b, g out)", lambda: ot.sgd_step(table, LR, 0.9, 0.0, True, coef, None, True), 6),
            ("sums, then step: the step alone", None, 6))
    parts = []
    for name, call, streams in rows:
        if call is None:
            t = [event_ms(rows[2][1], lambda: (hip.refill(), rows[0][1]())) for _ in range(RUNS)]
        else:
            for _ in range(WARMUP):
                call()
            t = [event_ms(call, hip.refill if streams else None) for _ in range(RUNS)]
        m = float(np.median(t))
        parts.append(f"{name} {m:.3f} ms" + (f" = {streams * n * 4 / m / 1e9:.2f} TB/s" if streams else ""))
    lines.append("  hip entries alone: " + "; ".join(parts) + "   (the refill in front of `step` leaves the gradients freshly written; the last figure has the "
                 "sums pass between the refill and the step, as a training step does)")
    ok = med["hip"] < med["ref"]
    lines.append(f"  hip < ref: {'yes' if ok else 'NO'} ({med['ref'] / med['hip']:.1f}x)")
    return ok, drift


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "optim_ab.txt")
    aoc_amd._lib.lib()
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = [f"# One training update (clip_grad_norm_ {MAX_NORM}, SGD lr {LR} momentum 0.9 nesterov, weight decay {WD} except the betas, gradients zeroed): arms "
             f"alternating in one process; median [min, max] of {RUNS} after {WARMUP} warm-up steps; torch {torch.__version__}",
             f"# device: {torch.cuda.get_device_name(0)}"]
    failed = []
    dec = decoder_shapes()
    for title, shapes in (("decoder + DynamicPreHead + embedding head", dec), ("ResNet-101-shaped backbone + the same", resnet101_shapes() + dec)):
        with torch.no_grad():
            ok, drift = bench_list(title, shapes, gen, lines)
        if not ok:
            failed.append(f"{title}: the hip arm's median is not below the reference construction's")
        if not drift <= DRIFT_TOL:
            failed.append(f"{title}: the arms' parameters differ by {drift:.1e} of the largest, tolerance {DRIFT_TOL:.0e}")
        torch.cuda.empty_cache()
    lines += ["# FAILED: " + f for f in failed]
    print("\n".join(lines), flush=True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    for f in failed:
        print("FAILED: " + f, file=sys.stderr)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
