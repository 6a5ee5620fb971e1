"""References and bounds for the training update (csrc/optim.hip, aoc_amd.optim_train), shared by tests/test_optim_host.py and
tests/test_gpu_optim.py.  numpy and float64 only; no constant is fitted to output.

Three things live here.

1. The float32 RESTATEMENT of the kernels (``step32``, ``chunk_sumsq32``, ``finish64``): numpy float32 arithmetic rounds every operation once,
   as the library does (-ffp-contract=off).  The update is element-wise, so ``step32`` at the coefficient the device produced is EXACT: the
   GPU tests ask for its bits.  ``chunk_sumsq32`` repeats the stated order of a chunk's sum (thread t of 256 owns the floats 1024 j + 4 t .. + 3,
   ascending address; the xor butterfly 32 .. 1; the waves ascending), ``finish64`` the double sum.

2. The float64 REFERENCE with a bound (``clip_sgd_ref``): a running error analysis of the five expressions

       g' = g * coef;  d = g' + wd * p (wd != 0);  b' = momentum * b + (1 - dampening) * d (a buffer exists) or d;
       v = d + momentum * b' (nesterov) or b';  p' = p + (-lr) * v

   carried by the class ``E`` (a value and what a float32 evaluation of it is off by at most): every rounded operation adds U = 2^-24 of the
   magnitude of its actual result, plus 2^-150 for a result in the subnormal range.  The hyperparameters enter as the float32 values both
   implementations hand to their kernels; ``1 - dampening`` carries 2 U (torch rounds the double difference, the library the float32 one).
   A fused a + alpha * b (torch fuses in some paths) rounds once where the analysis allows two, so it stays inside.
   The norm: a chunk's sum of squares passes every term through one product and at most 16 + 6 + 3 additions (16 per thread, 6 butterfly
   levels, 3 wave additions), all terms non-negative: relative gamma(26).  The double sum adds (ceil(n_chunks / 256) + 9) 2^-53.  The root
   moves by at most dS / sqrt(S), is rounded in double and then to float32.  The coefficient max_norm / (total_norm + 1e-6f) is carried by E
   with ONE MORE rounding than the kernel's quotient has, because torch forms it as reciprocal times max_norm; min(1, .) moves no error up.
   Every reference is taken at the float32 state a step actually received, so nothing is carried from step to step.

3. The SLIPS: ``clip_sgd_ref(..., slip=name)`` is the same function with one deliberate mistake; the tests demand that each leaves the bound.
"""
import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -150                       # half the smallest subnormal: what a rounding into the subnormal range is off by at most
CHUNK, THREADS = 4096, 256
SLIPS = ("wd_before_clip", "nesterov_old_buffer", "unclamped", "no_eps", "dampening_first", "dampening_dropped")
SIZES = (0, 1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8193, 3 * 4096)


def gamma(k):
    return k * U / (1.0 - k * U)


def rng(*seed):
    return np.random.RandomState(list(seed))


class E:
    """value v (float64 array) and a bound e >= |float32 evaluation - v|"""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, f64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, f64)

    @staticmethod
    def _r(v, e):                                         # one rounding of the computed value
        return E(v, e + U * (np.abs(v) + e) + TINY)

    def __mul__(self, o):
        return E._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __add__(self, o):
        return E._r(self.v + o.v, self.e + o.e)

    def __truediv__(self, o):
        lo = np.maximum(np.abs(o.v) - o.e, 1e-300)        # the denominator's smallest magnitude
        return E._r(self.v / o.v, (self.e + np.abs(self.v / o.v) * o.e) / lo)

    def neg(self):
        return E(-self.v, self.e)

    def more(self, k=1):                                  # k further roundings of the same value
        out = self
        for _ in range(k):
            out = E._r(out.v, out.e)
        return out


def check(got, want, tol):
    """max |got - want| / tol over the elements (0 / 0 counts as 0; a NaN or inf on either side counts as inf unless both sides agree)."""
    got, want, tol = np.asarray(got, f64).reshape(-1), np.asarray(want, f64).reshape(-1), np.asarray(tol, f64).reshape(-1)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want)
        ratio = np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    ratio = np.where(same, 0.0, np.where(np.isfinite(ratio), ratio, np.inf))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------ chunks
def chunk_prefix(sizes):
    """chunk_begin of every tensor and the number of chunks, by the rule: ceil(n / CHUNK) chunks per tensor, none for an empty one"""
    begins, at = [], 0
    for n in sizes:
        begins.append(at)
        at += -(-int(n) // CHUNK)
    return begins, at


def chunk_owner_brute(sizes):
    """the tensor of every chunk, one element at a time: chunk c of the list holds the elements [CHUNK k, CHUNK (k + 1)) of its tensor"""
    owner = []
    for i, n in enumerate(sizes):
        seen = set()
        for el in range(int(n)):
            seen.add(el // CHUNK)
        owner += [i] * len(seen)
    return owner


# ------------------------------------------------------------------------------------------ the float32 restatement
def chunk_sumsq32(x):
    """Sum of squares of one chunk (at most CHUNK float32 values) in the kernel's order, as a double."""
    x = np.asarray(x, f32).reshape(-1)
    assert x.size <= CHUNK
    pad = np.zeros(CHUNK, f32)
    pad[:x.size] = x
    lanes = pad.reshape(CHUNK // (4 * THREADS), THREADS, 4)            # [j, t, k]: float 1024 j + 4 t + k
    acc = np.zeros(THREADS, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(lanes.shape[0]):
            for k in range(4):
                acc = acc + lanes[j, :, k] * lanes[j, :, k]
        w = acc.reshape(THREADS // 64, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[:, lane ^ o]
        s = ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]
    return f64(s)


def partials32(grads, sizes=None):
    """the chunk sums of a list of gradients in table order; grads[i] None: tensor i (of sizes[i] elements) has no gradient, its chunks give 0.0"""
    out = []
    for i, g in enumerate(grads):
        if g is None:
            out += [0.0] * (-(-int(sizes[i]) // CHUNK))
            continue
        flat = np.asarray(g, f32).reshape(-1)
        out += [chunk_sumsq32(flat[c:c + CHUNK]) for c in range(0, flat.size, CHUNK)]
    return np.asarray(out, f64)


def finish64(partial, max_norm):
    """(total_norm, coef) as float32 from the chunk sums, in the finish kernel's order"""
    partial = np.asarray(partial, f64)
    acc = np.zeros(THREADS, f64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for i in range(0, partial.size, THREADS):
            row = partial[i:i + THREADS]
            acc[:row.size] = acc[:row.size] + row
        w = acc.reshape(THREADS // 64, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[:, lane ^ o]
        s = ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]
        norm = f32(np.sqrt(s))
        c = f32(max_norm) / (norm + f32(1e-6))
        coef = f32(1.0) if c > f32(1.0) else f32(c)
    return norm, coef


def step32(g, p, b, coef, wd, lr, momentum, dampening, nesterov):
    """One update of one tensor in float32, one rounding per operation: (p', b').  b None: no buffer yet; b' None when momentum == 0."""
    g, p = np.asarray(g, f32), np.asarray(p, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = g * f32(coef)
        if f32(wd) != 0:
            d = d + p * f32(wd)
        nb, v = None, d
        if f32(momentum) != 0:
            nb = np.asarray(b, f32) * f32(momentum) + d * (f32(1.0) - f32(dampening)) if b is not None else d
            v = d + nb * f32(momentum) if nesterov else nb
        return p + v * (-f32(lr)), nb


# ------------------------------------------------------------------------------------------ the float64 reference and its bound
def norm_ref(grads, sizes=None):
    """(S, dS, N, dN): the float64 sum of squares and norm of the gradients, and what the kernels' are off by at most"""
    flats = [np.asarray(g, f64).reshape(-1) for g in grads if g is not None]
    n = int(sum(x.size for x in flats))
    n_chunks = chunk_prefix([x.size for x in flats])[1] if sizes is None else chunk_prefix(sizes)[1]
    S = float(sum(float(np.dot(x, x)) for x in flats))
    dS = gamma(1 + 16 + 6 + 3) * S + n * 2.0 ** -149 + (-(-n_chunks // THREADS) + 9) * 2.0 ** -53 * S
    N = float(np.sqrt(S))
    dN = 0.0 if S == 0 else dS / N
    dN = dN + 2.0 ** -53 * N + U * (N + dN) + TINY        # the root in double, then its rounding to float32
    return S, dS, N, dN


def coef_ref(N, dN, max_norm, slip=None):
    """E of min(1, max_norm / (N + 1e-6f)); max_norm None: no clip, exactly 1"""
    if max_norm is None:
        return E(1.0)
    den = E(N, dN) if slip == "no_eps" else E(N, dN) + E(f64(f32(1e-6)))
    c = (E(f64(f32(max_norm))) / den).more(1)             # torch: reciprocal times max_norm, one more rounding than the quotient
    if slip == "unclamped":
        return c
    return E(np.minimum(c.v, 1.0), c.e)


def step_ref(g, p, b, coef, wd, lr, momentum, dampening, nesterov, slip=None):
    """(p' as E, b' as E or None) of one tensor from its float32 state, widened; coef an E"""
    g, p = E(np.asarray(g, f64)), E(np.asarray(p, f64))
    wdE, lrE, mE = E(f64(f32(wd))), E(f64(f32(lr))), E(f64(f32(momentum)))
    omd = f64(1.0) - f64(f32(dampening))
    omdE = E(omd, 2 * U * abs(omd))
    if slip == "wd_before_clip":
        d = (g + wdE * p) * coef if f32(wd) != 0 else g * coef
    else:
        d = g * coef
        if f32(wd) != 0:
            d = d + wdE * p
    nb, v = None, d
    if f32(momentum) != 0:
        if b is not None:
            bE = E(np.asarray(b, f64))
            nb = mE * bE + (d if slip == "dampening_dropped" else (d if omd == 1.0 else omdE * d))
        else:
            nb = omdE * d if slip == "dampening_first" else d
        if nesterov:
            old = E(np.asarray(b, f64)) if b is not None else E(np.zeros_like(d.v))
            v = d + mE * (old if slip == "nesterov_old_buffer" else nb)
        else:
            v = nb
    return p + lrE.neg() * v, nb


def clip_sgd_ref(grads, params, bufs, wds, lrs, max_norm, momentum, dampening, nesterov, slip=None):
    """One step of a list of tensors.  grads[i] None: the tensor is skipped (its entry of the result is None).  Returns
    (N, dN, coef as E, [(p' as E, b' as E or None) or None])."""
    _, _, N, dN = norm_ref(grads)
    coef = coef_ref(N, dN, max_norm, slip)
    out = []
    for g, p, b, wd, lr in zip(grads, params, bufs, wds, lrs):
        out.append(None if g is None else step_ref(g, p, b, coef, wd, lr, momentum, dampening, nesterov, slip))
    return N, dN, coef, out


# ------------------------------------------------------------------------------------------ inputs
def make_list(sizes, seed, scale=1.0):
    """(grads, params) float32 lists; the sizes may include 0"""
    r = rng(seed)
    grads = [(scale * r.standard_normal(n)).astype(f32) for n in sizes]
    params = [r.standard_normal(n).astype(f32) for n in sizes]
    return grads, params


HOST_SIZES = (5, 0, 257, 4097, 1, 33, 4096, 700, 3, 129)            # ten tensors, an empty one included
MODES = {"nesterov": dict(momentum=0.9, dampening=0.0, nesterov=True, wd=1e-4),
         "momentum": dict(momentum=0.9, dampening=0.0, nesterov=False, wd=1e-4),
         "plain": dict(momentum=0.0, dampening=0.0, nesterov=False, wd=1e-4),
         "dampening": dict(momentum=0.9, dampening=0.1, nesterov=False, wd=1e-4),
         "no_wd": dict(momentum=0.9, dampening=0.0, nesterov=True, wd=0.0)}
