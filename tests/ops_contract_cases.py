"""The tensor contract of aoc_amd.ops (the only module that hands addresses to libaoc_hip.so), as data: one small canonical call per public
callable, the role of every tensor it takes, the variants of those tensors an integrator may pass, and the recorder that watches what reaches
the library.  Shared by tests/test_ops_contract_host.py (CPU, no library: a stub stands in for it) and tests/test_gpu_ops_contract.py.

The contract (ops.py module docstring, INTEGRATION.md "Behavioural notes"):
  * inputs of another dtype or layout are converted (or refused) -- never misread;
  * caller-provided outputs are never converted: contiguous, exact dtype and shape, or an exception before anything is enqueued;
  * every tensor whose address is taken lives until the library call that reads the address has been made.

Every variant tensor's storage, counted from its address, covers at least the bytes of the canonical one, so even a front-end that handed
it over unconverted could not make a kernel leave an allocation; the narrower dtypes are host-only (NARROW)."""
import ctypes
import weakref

import numpy as np
import torch

F, I, OUT, WS = "float input", "integer input", "caller-provided output", "workspace"

# callables that take no device tensor (checked by test_ops_contract_host.py::test_every_public_callable_is_listed: none of them may have a case,
# none of them may reach _p / _addr)
EXEMPT = {
    "kmeans_init_rows_draw": "host function: numpy arrays and a numpy RandomState in, numpy arrays out",
    "split_record_bytes": "a host query (C -> bytes per record)",
    "dense_prune_stats": "reads the library's host-side developer counters",
    "set_stream_cus": "sets a host-side integer of the library",
    "inference_only": "inspects requires_grad only; no address is taken",
}

ERRORS = (TypeError, ValueError, AssertionError)      # + _lib.AocHipError, added by the tests (the package is imported there)


# ------------------------------------------------------------------------------------------ the recorder and the stub library
class Record:
    __slots__ = ("shape", "dtype", "contiguous", "device", "numel", "ref", "alive", "mod16")


class Recorder:
    """Wraps ops._p and ops._addr: at the moment an address is taken it notes shape, dtype, contiguity, device, the address modulo 16 (the
    alignment contract, tests/alignment_cases.py) and a weakref of the tensor.
    The stub library calls entered(): every address taken since the previous library call must still belong to a live tensor THEN."""

    def __init__(self):
        self.records, self.pending, self.calls = [], [], []

    def note(self, t):
        r = Record()
        if t is None:
            r.shape = None
        else:
            r.shape, r.dtype, r.contiguous, r.device, r.numel = tuple(t.shape), t.dtype, t.is_contiguous(), t.device, t.numel()
            r.ref, r.alive, r.mod16 = weakref.ref(t), None, t.data_ptr() % 16
            self.pending.append(r)
        self.records.append(r)

    def entered(self, name):
        self.calls.append(name)
        for r in self.pending:
            r.alive = r.ref() is not None
        self.pending = []


HOST_QUERIES = {"aoc_frame_channels": 24, "aoc_cluster_chain_layout": 0}       # host functions of the library that enqueue nothing


class StubLib:
    """libaoc_hip.so's stand-in: *_bytes functions return a small size, the host queries a plausible value, every other aoc_* function
    records the call and returns 0 (AOC_OK).  Nothing is launched."""

    def __init__(self, recorder):
        self._rec = recorder

    def __getattr__(self, name):
        if not name.startswith("aoc_"):
            raise AttributeError(name)
        if name == "aoc_split_record_bytes":
            return lambda C: 448 if (C % 4 == 0 and 0 < C <= 100) else 0
        if name.endswith("_bytes"):
            return lambda *a: 1 << 20
        if name in HOST_QUERIES:
            return lambda *a, _v=HOST_QUERIES[name]: _v

        def call(*a):
            self._rec.entered(name)
            return 0
        return call


def install(monkeypatch, ops, stub=True):
    """Wraps _p / _addr of `ops`; with stub also replaces the library, _need_gpu and _stream.  -> the Recorder."""
    rec = Recorder()
    real_p, real_addr = ops._p, ops._addr                  # (both must exist: an address that left some other way would go unseen)

    def p(t):
        rec.note(t)
        return real_p(t)

    def addr(t):
        rec.note(t)
        return real_addr(t)
    monkeypatch.setattr(ops, "_p", p)
    monkeypatch.setattr(ops, "_addr", addr)
    if stub:
        lib = StubLib(rec)
        monkeypatch.setattr(ops._lib, "lib", lambda: lib)
        monkeypatch.setattr(ops, "_need_gpu", lambda *t: None)
        monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(0))
        monkeypatch.setattr(ops, "_corr_ws", {})
    return rec


def run_recorded(ops, case, a, errors):
    """One call of `case` under an installed recorder's patches -> (exception or None, result)."""
    try:
        return None, case.call(ops, a)
    except errors as e:
        return e, None


def check_rule(canon, rec, err, role, device):
    """The host rule for one variant run.  canon: the canonical run's records.  -> a list of complaints (empty = the variant passes)."""
    if err is not None:
        return [f"raised {type(err).__name__} AFTER the library had been called ({rec.calls})"] if rec.calls else []
    if role == OUT:
        return ["a caller-provided output of another dtype / layout / size was accepted (outputs are never converted: it must raise)"]
    bad = []
    if len(rec.records) != len(canon):
        return [f"{len(rec.records)} addresses taken, the canonical call takes {len(canon)}"]
    for k, (c, r) in enumerate(zip(canon, rec.records)):
        if (c.shape is None) != (r.shape is None):
            bad.append(f"pointer {k}: None-ness differs")
        elif c.shape is not None:
            if not r.contiguous:
                bad.append(f"pointer {k}: non-contiguous {r.shape}")
            if r.dtype != c.dtype:
                bad.append(f"pointer {k}: {r.dtype} where the library reads {c.dtype}")
            if r.numel < c.numel:
                bad.append(f"pointer {k}: {r.numel} elements, the canonical call hands over {c.numel}")
            if r.device.type != torch.device(device).type:
                bad.append(f"pointer {k}: on {r.device}")
            if r.alive is False:
                bad.append(f"pointer {k}: the tensor {r.shape} was freed before the library call (a converted temporary)")
            if r.alive is None:
                bad.append(f"pointer {k}: address taken but no library call followed")
    return bad


# ------------------------------------------------------------------------------------------ variants
def strided(t, fill=None):
    """Equal values, every second element of the last axis of a buffer twice as wide."""
    buf = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    if fill is not None:
        buf.fill_(fill)
    v = buf[..., ::2]
    v.copy_(t)
    return v


def short(t):
    """One element short of the right shape, inside a full-size storage."""
    return t.clone().reshape(-1)[:t.numel() - 1]


def wide(t):
    return t.double() if t.dtype.is_floating_point else t.long()


VARIANTS = {                       # role -> {variant name: transform}; the first four groups of the issue, used on the host and on the device
    F: {"float64": lambda t: t.double(), "strided": strided},
    I: {"int64": lambda t: t.long(), "strided": strided},
    OUT: {"strided": strided, "wide dtype": wide, "one short": short},
}
NARROW = {                         # host only: a kernel that read these unconverted would leave the allocation
    F: {"half": lambda t: t.half(), "bool": lambda t: t > 0},
    I: {"uint8": lambda t: t.to(torch.uint8), "int16": lambda t: t.to(torch.int16)},
}


def variants_of(case, narrow=False):
    """-> [(label, {argument: transform}, role)]: each input one at a time, then all float inputs / all integer inputs at once."""
    out = []
    for role, table in VARIANTS.items():
        names = [n for n, r in case.roles.items() if r == role]
        for vname, fn in table.items():
            for n in names:
                out.append((f"{n}:{vname}", {n: fn}, role))
            if role != OUT and len(names) > 1 and vname != "strided":
                out.append((f"all {role}s:{vname}", {n: fn for n in names}, role))
    if narrow:
        for role, table in NARROW.items():
            for vname, fn in table.items():
                for n in (n for n, r in case.roles.items() if r == role):
                    out.append((f"{n}:{vname}", {n: fn}, role))
    return out


def apply_variant(a, transforms):
    a = dict(a)
    for n, fn in transforms.items():
        a[n] = fn(a[n])
    return a


# ------------------------------------------------------------------------------------------ shared operands
def _rs(seed):
    return np.random.RandomState(seed)


def fl(rng, *shape, scale=1.0):
    return torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32))


def _to(a, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in a.items()}


PREP_FIELDS = ("right_bits", "wrong_bits", "fg_rows", "obj_rows", "counts", "obj_offsets")
POOL = dict(h=6, w=8, C=100, O=3, m=40, kmax=4)           # one 6 x 8 pool frame, 40 query pixels, C = 100 (the split records need C % 4 == 0)


def _host_prep(lab):
    """numpy stand-in of aoc_label_prep for the stubbed host runs (shapes and dtypes are what matters there)."""
    n, O = lab.shape
    hard = lab > 0.5
    kept = hard.any(1)
    right = np.zeros(n, np.uint32)
    for o in range(O):
        right |= hard[:, o].astype(np.uint32) << np.uint32(o)
    wrong = (~right) & np.uint32((1 << O) - 1)
    right |= kept.astype(np.uint32) << np.uint32(31)
    rows = [np.nonzero(hard[:, o])[0] for o in range(O)]
    obj_rows = np.zeros(n * O, np.int32)
    packed = np.concatenate(rows)
    obj_rows[:packed.size] = packed
    counts = np.array([len(r) for r in rows] + [int(kept.sum())], np.int32)
    fg = np.zeros(n, np.int32)
    fg[:int(kept.sum())] = np.nonzero(kept)[0]
    offs = np.concatenate([[0], np.cumsum(counts[:O])]).astype(np.int32)
    return dict(right_bits=torch.from_numpy(right.view(np.int32).copy()), wrong_bits=torch.from_numpy(wrong.view(np.int32).copy()),
                fg_rows=torch.from_numpy(fg), obj_rows=torch.from_numpy(obj_rows), counts=torch.from_numpy(counts), obj_offsets=torch.from_numpy(offs))


_SCENE = {}


def scene(ops, device):
    """The operands the matching cases share, computed ONCE per device and never modified (every case clones what it hands over): a labelled
    pool, its label prep, one k-means chain, the proxies, and the forward results the backward calls differentiate.  On the device the
    library computes them (so every row index a kernel follows is one the library produced); on the host (stubbed library) stand-ins of the
    same shapes and dtypes."""
    key = torch.device(device).type
    if key in _SCENE:
        return _SCENE[key]
    P = POOL
    h, w, C, O, m, kmax = (P[k] for k in ("h", "w", "C", "O", "m", "kmax"))
    n = h * w
    rng = _rs(11)
    s = dict(n=n)
    s["pool"] = fl(rng, n, C, scale=0.1).abs()
    s["query"] = fl(rng, m, C, scale=0.1).abs()
    lab = np.zeros((n, O), np.float32)
    lab[np.arange(n), np.arange(n) * 7 % O] = 1.0
    lab[[1, 4, 2, 5, 8]] = 0.0                                 # a few unlabelled rows: 16, 14 and 13 rows per object (the sticky K falls)
    s["labels"] = torch.from_numpy(lab)
    s["bias"] = torch.tensor([0.25, -0.5, 0.125])
    counts = [int(lab[:, o].sum()) for o in range(O)]
    init = np.stack([_rs(3 + o).permutation(counts[o])[:kmax] for o in range(O)]).astype(np.int32)
    s["init_rows"] = torch.from_numpy(init)
    s["total"] = int(sum(counts))
    s["grad_planes"] = fl(rng, O, m)
    if key == "cuda":
        s = _to(s, device)
        prep = ops.label_prep(s["labels"])
        for f in PREP_FIELDS:
            s[f] = getattr(prep, f)
        # the chain as matching.cluster_proxies drives it (one level: the replicated row list is the prep's own)
        _, s["seg_offsets"], s["seg_k"] = ops.kmeans_replicate_levels(prep.obj_rows, prep.obj_offsets, O, 1, [kmax], rows_capacity=prep.obj_rows.numel())
        s["centroids"], s["klabels"], s["ccounts"] = ops.kmeans_segmented(s["pool"], prep.obj_rows, s["seg_offsets"], s["seg_k"], s["init_rows"], kmax)
        s["proxies"], s["proxy_sqnorm"] = ops.build_proxies(s["pool"], prep.fg_rows, s["seg_offsets"], s["seg_k"], s["klabels"], s["centroids"])
        s["dense_T"] = torch.empty(O, m, device=device)
        s["dense_arg"] = torch.empty(O, m, dtype=torch.int32, device=device)
        ops.dense_match_argmin(s["query"], s["pool"], prep, s["bias"], s["dense_T"], s["dense_arg"], 1, m)
        s["k1"] = s["centroids"][:, 0].contiguous()
        s["k1_T"] = torch.empty(O, m, device=device)
        ops.proxy_corr_min(s["query"], s["k1"], None, list(range(O)), [1] * O, [o * m for o in range(O)], s["bias"], s["k1_T"], 1)
        sb, ss, so = set_lists()
        s["set_T"] = torch.empty(2 * O, m, device=device)
        s["set_arg"] = torch.empty(2 * O, m, dtype=torch.int32, device=device)
        ops.proxy_set_match_argmin(s["query"], s["proxies"].reshape(-1, C), s["proxy_sqnorm"].reshape(-1), sb, ss, so, set_bias(s["bias"]), s["set_T"],
                                   s["set_arg"], 1)
        qs = ops.split_rows(s["query"], tiled=True)
        s["q_records"], s["q_sqnorm"], s["overflow"] = qs.records, qs.sqnorm, qs.overflow
        ps = ops.split_rows(s["pool"], overflow=qs.overflow)
        s["p_records"], s["p_sqnorm"] = ps.records, ps.sqnorm
        torch.cuda.synchronize()
    else:
        s.update(_host_prep(lab))
        s["seg_k"], s["seg_offsets"] = torch.full((O,), kmax, dtype=torch.int32), s["obj_offsets"].clone()
        s["centroids"] = fl(rng, O, kmax, C)
        s["klabels"] = torch.from_numpy((np.arange(n * O) % kmax).astype(np.int32))
        s["ccounts"] = torch.ones(O, kmax, dtype=torch.int32)
        s["proxies"], s["proxy_sqnorm"] = fl(rng, O, 2, kmax, C), fl(rng, O, 2, kmax).abs()
        s["dense_T"], s["dense_arg"] = fl(rng, O, m), torch.from_numpy((np.arange(O * m) % n).astype(np.int32).reshape(O, m))
        s["k1"], s["k1_T"] = s["centroids"][:, 0].contiguous(), fl(rng, O, m)
        s["set_T"], s["set_arg"] = fl(rng, 2 * O, m), torch.from_numpy((np.arange(2 * O * m) % kmax).astype(np.int32).reshape(2 * O, m))
        s["q_records"], s["q_sqnorm"] = torch.zeros((m + 31) // 32 * 32, 448, dtype=torch.uint8), fl(rng, m).abs()
        s["p_records"], s["p_sqnorm"] = torch.zeros(n, 448, dtype=torch.uint8), fl(rng, n).abs()
        s["overflow"] = torch.zeros(1, dtype=torch.int32)
    _SCENE[key] = s
    return s


def set_lists():
    """(set_begin, set_size, set_out_offset) of the 2 O proxy sets (centroid | centroid_avg per object) over POOL's proxy table."""
    O, kmax, m = POOL["O"], POOL["kmax"], POOL["m"]
    sets = [(o, f) for o in range(O) for f in range(2)]
    return [(o * 2 + f) * kmax for o, f in sets], [kmax] * len(sets), [i * m for i in range(len(sets))]


def set_bias(bias):
    return bias.repeat_interleave(2)


def take(s, *names, **renamed):
    """Clones of scene tensors under their own (or new) names: a case never hands the shared operands to a call."""
    a = {k: s[k].clone() for k in names}
    a.update({new: s[old].clone() for new, old in renamed.items()})
    return a


def mk_prep(ops, a):
    p = ops.LabelPrep()
    p.n, p.n_obj = POOL["h"] * POOL["w"], POOL["O"]
    for f in PREP_FIELDS:
        setattr(p, f, a[f])
    return p


def mk_split(ops, records, sqnorm, overflow, n, tiled):
    r = ops.SplitRows()
    r.records, r.sqnorm, r.overflow, r.n, r.tiled = records, sqnorm, overflow, n, tiled
    return r


PREP_ROLES = {f: I for f in PREP_FIELDS}
SENTINEL = {torch.float32: 12345.5, torch.float64: 12345.5, torch.int32: -77, torch.int64: -77, torch.uint8: 201}


def blank(device, shape, dtype=torch.float32):
    """A caller-provided output, pre-filled with the sentinel the device test looks for after a refused call."""
    return torch.full(tuple(shape), SENTINEL[dtype], dtype=dtype, device=device)


# ------------------------------------------------------------------------------------------ the registry
class Case:
    def __init__(self, name, covers, build, roles, call, collect):
        self.name, self.covers, self.build, self.roles, self.call, self.collect = name, tuple(covers), build, roles, call, collect


CASES = {}


def _as_list(res, a):
    return list(res) if isinstance(res, (tuple, list)) else [res]


def simple(name, roles, make, call, collect=_as_list, covers=None):
    """Registers a case: make(ops, device) -> the named arguments (seeded; moved to the device here), roles of the tensors among them,
    call(ops, a) -> result, collect(result, a) -> the output tensors to compare."""
    CASES[name] = Case(name, covers or [name], lambda ops, device: _to(make(ops, device), device), roles, call, collect)


def outs(*names):
    return lambda res, a: [a[n] for n in names]


def _seq(res, a):
    return [t for t in res if t is not None]


# ---- labels and k-means
simple("label_bits", {"labels": F}, lambda ops, d: take(scene(ops, d), "labels"), lambda ops, a: ops.label_bits(a["labels"]))
simple("label_prep", {"labels": F}, lambda ops, d: take(scene(ops, d), "labels"), lambda ops, a: ops.label_prep(a["labels"]),
       lambda r, a: [r.right_bits, r.wrong_bits, r.counts, r.obj_offsets, r.fg_rows[:int(r.counts[-1])], r.obj_rows[:int(r.obj_offsets[-1])]],
       covers=["label_prep", "LabelPrep"])
simple("kmeans_plan", {"counts": I}, lambda ops, d: take(scene(ops, d), "counts"), lambda ops, a: ops.kmeans_plan(a["counts"], POOL["O"], 15))
KM_ROLES = {"pool": F, "obj_rows": I, "seg_offsets": I, "seg_k": I, "init_rows": I}
simple("kmeans_segmented", KM_ROLES, lambda ops, d: dict(take(scene(ops, d), *KM_ROLES), total=scene(ops, d)["total"]),
       lambda ops, a: ops.kmeans_segmented(a["pool"], a["obj_rows"], a["seg_offsets"], a["seg_k"], a["init_rows"], POOL["kmax"]),
       lambda r, a: [r[0], r[1][:a["total"]], r[2]])
REP_ROLES = {"obj_rows": I, "seg_offsets": I, "seg_k": I}
simple("kmeans_replicate", REP_ROLES, lambda ops, d: dict(take(scene(ops, d), *REP_ROLES), total=scene(ops, d)["total"], seg_k=torch.tensor([4, 3, 4], dtype=torch.int32)),
       lambda ops, a: ops.kmeans_replicate(a["obj_rows"], a["seg_offsets"], a["seg_k"], 2), lambda r, a: [r[0][:a["total"]], r[1], r[2]])
simple("kmeans_replicate_levels", {"obj_rows": I, "obj_offsets": I}, lambda ops, d: dict(take(scene(ops, d), "obj_rows", "obj_offsets"), total=scene(ops, d)["total"]),
       lambda ops, a: ops.kmeans_replicate_levels(a["obj_rows"], a["obj_offsets"], POOL["O"], 2, [4, 2]), lambda r, a: [r[0][:a["total"]], r[1], r[2]])
BP_ROLES = {"pool": F, "fg_rows": I, "seg_offsets": I, "seg_k": I, "klabels": I, "centroids": F}
simple("build_proxies", BP_ROLES, lambda ops, d: take(scene(ops, d), *BP_ROLES),
       lambda ops, a: ops.build_proxies(a["pool"], a["fg_rows"], a["seg_offsets"], a["seg_k"], a["klabels"], a["centroids"]))


# ---- correlation
def _corr_args(ops, d):
    s = scene(ops, d)
    a = take(s, "query", "proxy_sqnorm", table="proxies", set_bias="bias")
    a["table"], a["proxy_sqnorm"], a["set_bias"] = a["table"].reshape(-1, POOL["C"]), a["proxy_sqnorm"].reshape(-1), set_bias(a["set_bias"]).contiguous()
    a["out"] = blank(a["query"].device, (2 * POOL["O"], POOL["m"]))
    return a


CORR_ROLES = {"query": F, "table": F, "proxy_sqnorm": F, "set_bias": F, "out": OUT}
simple("proxy_corr_min", CORR_ROLES, _corr_args,
       lambda ops, a: ops.proxy_corr_min(a["query"], a["table"], a["proxy_sqnorm"], *set_lists(), a["set_bias"], a["out"], 1), outs("out"))
simple("proxy_corr_min_batched", CORR_ROLES, _corr_args,
       lambda ops, a: ops.proxy_corr_min_batched([(a["query"], a["table"], a["proxy_sqnorm"], a["set_bias"], a["out"])], *set_lists()), outs("out"))


def _rec_args(ops, d):
    return dict(_corr_args(ops, d), **take(scene(ops, d), "q_records", "q_sqnorm", "overflow"))


def _rec_call(cached):
    def call(ops, a):
        qs = mk_split(ops, a["q_records"], a["q_sqnorm"], a["overflow"], POOL["m"], True)
        cache = ops.CorrTableCache(a["query"].device) if cached else None
        return ops.proxy_corr_min_records([(a["query"], qs, a["table"], a["proxy_sqnorm"], a["set_bias"], a["out"])], *set_lists(), cache=cache)
    return call


REC_ROLES = dict(CORR_ROLES, q_records=WS, q_sqnorm=WS, overflow=WS)
simple("proxy_corr_min_records", REC_ROLES, _rec_args, _rec_call(False), outs("out"))
simple("proxy_corr_min_records(cache)", REC_ROLES, _rec_args, _rec_call(True), outs("out"), covers=["proxy_corr_min_records", "CorrTableCache"])
simple("proxy_set_match_argmin", dict(CORR_ROLES, arg=OUT),
       lambda ops, d: dict(_corr_args(ops, d), arg=blank(torch.device("cpu"), (2 * POOL["O"], POOL["m"]), torch.int32)),
       lambda ops, a: ops.proxy_set_match_argmin(a["query"], a["table"], a["proxy_sqnorm"], *set_lists(), a["set_bias"], a["out"], a["arg"], 1), outs("out", "arg"))


# ---- dense matching
def _dense_args(ops, d, *more, **renamed):
    a = take(scene(ops, d), "query", "pool", "bias", *PREP_FIELDS, *more, **renamed)
    a["out"] = blank(a["query"].device, (POOL["O"], POOL["m"]))
    return a


DENSE_ROLES = dict(PREP_ROLES, query=F, pool=F, bias=F, out=OUT)
simple("dense_match_min", DENSE_ROLES, _dense_args,
       lambda ops, a: ops.dense_match_min(a["query"], a["pool"], mk_prep(ops, a), a["bias"], a["out"], 1, POOL["m"]), outs("out"))
simple("dense_match_argmin", dict(DENSE_ROLES, arg=OUT), lambda ops, d: dict(_dense_args(ops, d), arg=blank(torch.device("cpu"), (POOL["O"], POOL["m"]), torch.int32)),
       lambda ops, a: ops.dense_match_argmin(a["query"], a["pool"], mk_prep(ops, a), a["bias"], a["out"], a["arg"], 1, POOL["m"]), outs("out", "arg"))
simple("dense_match", DENSE_ROLES, _dense_args,
       lambda ops, a: ops.dense_match(a["query"], a["pool"], mk_prep(ops, a), a["bias"], a["out"], 1, POOL["m"]), outs("out"))
SPLIT_WS = dict(q_records=WS, q_sqnorm=WS, p_records=WS, p_sqnorm=WS, overflow=WS)
simple("dense_match_min_split", dict(DENSE_ROLES, **SPLIT_WS), lambda ops, d: _dense_args(ops, d, *SPLIT_WS),
       lambda ops, a: ops.dense_match_min_split(a["query"], mk_split(ops, a["q_records"], a["q_sqnorm"], a["overflow"], POOL["m"], True), a["pool"],
                                                mk_split(ops, a["p_records"], a["p_sqnorm"], a["overflow"], POOL["h"] * POOL["w"], False), mk_prep(ops, a),
                                                a["bias"], a["out"], 1, POOL["m"]), outs("out"))


def _grads(device, **shapes):
    return {k: blank(device, v) for k, v in shapes.items()}


GRAD3 = {"grad_query": OUT, "grad_second": OUT, "grad_bias": OUT}
simple("dense_match_backward", dict(GRAD3, grad_out=F, T=F, arg=I, query=F, pool=F),
       lambda ops, d: dict(take(scene(ops, d), "query", "pool", grad_out="grad_planes", T="dense_T", arg="dense_arg"),
                           **_grads("cpu", grad_query=(POOL["m"], POOL["C"]), grad_second=(POOL["h"] * POOL["w"], POOL["C"]), grad_bias=(POOL["O"],))),
       lambda ops, a: ops.dense_match_backward(a["grad_out"], a["T"], a["arg"], 1, POOL["m"], a["query"], a["pool"], POOL["O"], grad_query=a["grad_query"],
                                               grad_pool=a["grad_second"], grad_bias=a["grad_bias"]), _seq)
simple("proxy_match_backward", dict(GRAD3, grad_out=F, T=F, query=F, k1=F),
       lambda ops, d: dict(take(scene(ops, d), "query", "k1", grad_out="grad_planes", T="k1_T"),
                           **_grads("cpu", grad_query=(POOL["m"], POOL["C"]), grad_second=(POOL["O"], POOL["C"]), grad_bias=(POOL["O"],))),
       lambda ops, a: ops.proxy_match_backward(a["grad_out"], a["T"], 1, POOL["m"], a["query"], a["k1"], grad_query=a["grad_query"],
                                               grad_proxies=a["grad_second"], grad_bias=a["grad_bias"]), _seq)


def _set_back_args(ops, d):
    s = scene(ops, d)
    a = take(s, "query", table="proxies", T="set_T", arg="set_arg")
    a["table"] = a["table"].reshape(-1, POOL["C"])
    a["grad_out"] = fl(_rs(5), 2 * POOL["O"], POOL["m"])
    a.update(_grads("cpu", grad_query=(POOL["m"], POOL["C"]), grad_second=(POOL["O"] * 2 * POOL["kmax"], POOL["C"]), grad_bias=(POOL["O"],)))
    return a


simple("proxy_set_match_backward", dict(GRAD3, grad_out=F, T=F, arg=I, query=F, table=F), _set_back_args,
       lambda ops, a: ops.proxy_set_match_backward(a["grad_out"], a["T"], a["arg"], 1, a["query"], a["table"], *set_lists(), [o for o in range(POOL["O"]) for _ in range(2)],
                                                   POOL["O"], grad_query=a["grad_query"], grad_proxies=a["grad_second"], grad_bias=a["grad_bias"]), _seq)
CAB_ROLES = {"grad_proxies": F, "fg_rows": I, "n_fg": I, "seg_offsets": I, "seg_k": I, "klabels": I, "grad_pool": OUT}
simple("centroid_avg_backward", CAB_ROLES,
       lambda ops, d: dict(take(scene(ops, d), "fg_rows", "seg_offsets", "seg_k", "klabels"), n_fg=scene(ops, d)["counts"][POOL["O"]:].clone(),
                           grad_proxies=fl(_rs(6), POOL["O"], 2, POOL["kmax"], POOL["C"]), grad_pool=blank("cpu", (POOL["h"] * POOL["w"], POOL["C"]))),
       lambda ops, a: ops.centroid_avg_backward(a["grad_proxies"], a["fg_rows"], a["n_fg"], a["seg_offsets"], a["seg_k"], a["klabels"], POOL["h"] * POOL["w"],
                                                grad_pool=a["grad_pool"]), outs("grad_pool"))

# ---- split records
simple("split_rows", {"x": F}, lambda ops, d: take(scene(ops, d), x="query"), lambda ops, a: ops.split_rows(a["x"]),
       lambda r, a: [r.records, r.sqnorm])
simple("split_rows(tiled)", {"x": F, "overflow": OUT}, lambda ops, d: dict(take(scene(ops, d), x="query"), overflow=torch.zeros(1, dtype=torch.int32)),
       lambda ops, a: ops.split_rows(a["x"], overflow=a["overflow"], tiled=True), lambda r, a: [r.records[:POOL["m"]], r.sqnorm], covers=["split_rows"])
simple("split_rows(out)", {"x": F, "records": OUT, "sqnorm": OUT, "overflow": OUT},
       lambda ops, d: dict(take(scene(ops, d), x="query"), records=blank("cpu", (POOL["m"], 448), torch.uint8), sqnorm=blank("cpu", (POOL["m"],)),
                           overflow=torch.zeros(1, dtype=torch.int32)),
       lambda ops, a: ops.split_rows(a["x"], out=mk_split(ops, a["records"], a["sqnorm"], a["overflow"], POOL["m"], False), row0=0),
       outs("records", "sqnorm"), covers=["split_rows", "SplitRows"])

# ---- resize and local matching (C = 4, a 5 x 6 map, 3 objects, radii 1 and 2: the smallest shapes of the local-matching cases)
LH, LW, LC, LO, RADII = 5, 6, 4, 3, (1, 2)


def _local(ops, d):
    rng = _rs(21)
    lab = np.zeros((LH * LW, LO), np.float32)
    lab[np.arange(LH * LW), np.arange(LH * LW) * 5 % LO] = 1.0
    bits = _host_prep(lab)["right_bits"]
    return dict(query=fl(rng, LH, LW, LC, scale=0.3), prev=fl(rng, LH, LW, LC, scale=0.3), prev_b=fl(rng, LH, LW, LC, scale=0.3), right_bits=bits,
                bias=torch.tensor([0.2, -0.1, 0.05]), labels=torch.from_numpy(lab))


simple("resize_bilinear_hwc", {"x": F}, lambda ops, d: dict(x=fl(_rs(1), 3, 4, 5)), lambda ops, a: ops.resize_bilinear_hwc(a["x"], 5, 7))
simple("resize_bilinear_planes", {"x": F, "out": OUT}, lambda ops, d: dict(x=fl(_rs(2), 4, 3, 5), out=blank("cpu", (4, 5, 7))),
       lambda ops, a: ops.resize_bilinear_planes(a["x"], 5, 7, a["out"], 35, 1), outs("out"))
simple("resize_bilinear_planes_grouped", {"x": F, "out": OUT}, lambda ops, d: dict(x=fl(_rs(3), 2 * 3 * 2, 3, 5), out=blank("cpu", (2, 3, 2, 5, 7))),
       lambda ops, a: ops.resize_bilinear_planes_grouped(a["x"], 5, 7, a["out"], 2, 3, 3 * 2 * 35, 2 * 35, 35, 1), outs("out"))
simple("atrous_subsample", {"x": F}, lambda ops, d: dict(x=fl(_rs(4), 5, 7, 3)), lambda ops, a: ops.atrous_subsample(a["x"], 2))
simple("resize_nearest_bits", {"bits": I}, lambda ops, d: dict(bits=_local(ops, d)["right_bits"]),
       lambda ops, a: ops.resize_nearest_bits(a["bits"], LH, LW, 3, 4))
LOCAL_ROLES = {"query": F, "prev": F, "right_bits": I, "bias": F}
simple("local_window_match", LOCAL_ROLES, lambda ops, d: {k: _local(ops, d)[k] for k in LOCAL_ROLES},
       lambda ops, a: ops.local_window_match(a["query"], a["prev"], a["right_bits"], RADII, a["bias"], LO))
simple("local_window_match_argmin", dict(LOCAL_ROLES, out=OUT, arg=OUT),
       lambda ops, d: dict({k: _local(ops, d)[k] for k in LOCAL_ROLES}, out=blank("cpu", (LO, 2, LH, LW)), arg=blank("cpu", (LO, 2, LH, LW), torch.int32)),
       lambda ops, a: ops.local_window_match_argmin(a["query"], a["prev"], a["right_bits"], RADII, a["bias"], LO, out=a["out"], arg=a["arg"]))
simple("local_window_match_pair", dict(LOCAL_ROLES, prev_b=F), lambda ops, d: {k: _local(ops, d)[k] for k in dict(LOCAL_ROLES, prev_b=F)},
       lambda ops, a: ops.local_window_match_pair(a["query"], a["prev"], a["prev_b"], a["right_bits"], RADII, a["bias"], LO))


def _local_back_args(ops, d):
    a = {k: v.to(d) for k, v in _local(ops, d).items() if k in ("query", "prev", "right_bits", "bias")}
    if torch.device(d).type == "cuda":
        T, arg = ops.local_window_match_argmin(a["query"], a["prev"], a["right_bits"], RADII, a["bias"], LO)
    else:
        T, arg = fl(_rs(8), LO, 2, LH, LW), torch.zeros(LO, 2, LH, LW, dtype=torch.int32)
    a = dict(query=a["query"], prev=a["prev"], T=T, arg=arg, grad_out=fl(_rs(9), LO, 2, LH, LW))
    a.update(_grads("cpu", grad_query=(LH, LW, LC), grad_second=(LH, LW, LC), grad_bias=(LO,)))
    return a


simple("local_match_backward", dict(GRAD3, grad_out=F, T=F, arg=I, query=F, prev=F), _local_back_args,
       lambda ops, a: ops.local_match_backward(a["grad_out"], a["T"], a["arg"], a["query"], a["prev"], RADII[-1], grad_query=a["grad_query"],
                                               grad_prev=a["grad_second"], grad_bias=a["grad_bias"]), _seq)
LP_ROLES = {"cur": F, "prev": F, "labels": F, "prev_pos": F, "bias": F, "set_bias_out": OUT, "src": F, "dst": OUT}
simple("local_prep", LP_ROLES,
       lambda ops, d: dict(cur=_local(ops, d)["query"], prev=_local(ops, d)["prev"], labels=_local(ops, d)["labels"], prev_pos=fl(_rs(12), LO, LC),
                           bias=_local(ops, d)["bias"], set_bias_out=blank("cpu", (2 * LO + LO,)), src=fl(_rs(13), 10), dst=blank("cpu", (10,))),
       lambda ops, a: ops.local_prep(a["cur"], a["prev"], a["labels"], a["prev_pos"], 3, 4, obj_bias=a["bias"], n_pair_sets=2 * LO, set_bias_out=a["set_bias_out"],
                                     copies=((a["src"], a["dst"]),)), lambda r, a: list(r) + [a["set_bias_out"], a["dst"]])


def _proto_args(ops, d):
    rng = _rs(14)
    hw, n_ch = 7, 2 * 2 + 3
    feat = torch.from_numpy((rng.randint(0, 4, (LO, n_ch * hw)) * 0.5).astype(np.float32))
    return dict(feat=feat, prev_labels=torch.from_numpy(rng.uniform(0, 1, (hw, LO)).astype(np.float32)),
                **{k: fl(rng, LO, 5) for k in ("ref_pos", "ref_neg", "prev_pos", "prev_neg")})


simple("proto_finish", {"feat": OUT, "prev_labels": F, "ref_pos": F, "ref_neg": F, "prev_pos": F, "prev_neg": F}, _proto_args,
       lambda ops, a: ops.proto_finish(a["feat"], 7, 7 * 7, 0, 2, 2, 4, 5, 6, a["prev_labels"], a["ref_pos"], a["ref_neg"], a["prev_pos"], a["prev_neg"]),
       lambda r, a: [r, a["feat"]])

# ---- calibration side
simple("fg2bg_min", {"dis": F}, lambda ops, d: dict(dis=fl(_rs(15), 3, 2, 4, 5)), lambda ops, a: ops.fg2bg_min(a["dis"], 3))
simple("fg2bg_min(strided)", {"dis": F, "out": OUT}, lambda ops, d: dict(dis=fl(_rs(15), 3, 2 * 9 + 4), out=blank("cpu", (2 * 11 + 9,))),
       lambda ops, a: ops.fg2bg_min(a["dis"], 3, out=a["out"], dis_obj_stride=22, out_obj_stride=11, n_ch=2, inner=9),
       lambda r, a: [a["out"].reshape(-1)[:9], a["out"].reshape(-1)[11:20], a["out"].reshape(-1)[22:31]], covers=["fg2bg_min"])
simple("label_mix", {"labels": F, "rows": F}, lambda ops, d: dict(labels=fl(_rs(16), 9, 3).abs(), rows=fl(_rs(17), 3, 5)),
       lambda ops, a: ops.label_mix(a["labels"], a["rows"]))
MMP_ROLES = {"emb": F, "labels": F, "out_pos": OUT, "out_neg": OUT, "out_pos_sqnorm": OUT}
simple("masked_mean_pool", MMP_ROLES,
       lambda ops, d: dict(emb=fl(_rs(18), 2, 9, 5), labels=fl(_rs(19), 2, 3, 9).abs(), out_pos=blank("cpu", (3, 5)), out_neg=blank("cpu", (3, 5)),
                           out_pos_sqnorm=blank("cpu", (3,))),
       lambda ops, a: ops.masked_mean_pool(a["emb"], a["labels"], 1e-5, out_pos=a["out_pos"], out_neg=a["out_neg"], out_pos_sqnorm=a["out_pos_sqnorm"]),
       lambda r, a: [r[0], r[1], a["out_pos_sqnorm"]])
GATE = dict(N=3, c=5, D=6, H=4, W=3)


def _gate(seed, extra=0, **more):
    rng = _rs(seed)
    g = GATE
    a = dict(x=fl(rng, g["N"], g["c"], g["H"], g["W"]), head=fl(rng, g["N"], g["D"] + extra, scale=0.3), weight=fl(rng, g["c"], g["D"] + extra, scale=0.3),
             bias=fl(rng, g["c"], scale=0.1))
    a.update(more)
    return a


simple("film_gain", {"head": F, "weight": F, "bias": F}, lambda ops, d: {k: v for k, v in _gate(30).items() if k != "x"},
       lambda ops, a: ops.film_gain(a["head"], a["weight"], a["bias"]))
simple("channel_scale", {"x": F, "gain": F, "out": OUT}, lambda ops, d: dict(x=fl(_rs(31), 3, 5, 4, 3), gain=fl(_rs(32), 3, 5), out=blank("cpu", (3, 5, 4, 3))),
       lambda ops, a: ops.channel_scale(a["x"], a["gain"], out=a["out"]))
FS_ROLES = {"x": F, "head": F, "weight": F, "bias": F, "out": OUT}
simple("film_scale", FS_ROLES, lambda ops, d: _gate(33, out=blank("cpu", (3, 5, 4, 3))),
       lambda ops, a: ops.film_scale(a["x"], a["head"], a["weight"], a["bias"], out=a["out"]))
simple("cat_film_scale", dict(FS_ROLES, mem=F), lambda ops, d: _gate(34, x=fl(_rs(35), 3, 2, 4, 3), mem=fl(_rs(36), 3, 3, 4, 3), out=blank("cpu", (3, 5, 4, 3))),
       lambda ops, a: ops.cat_film_scale(a["x"], a["mem"], a["head"], a["weight"], a["bias"], out=a["out"]))
simple("cond_gate_pool", {"z": F, "phi_w": F, "phi_b": F}, lambda ops, d: dict(z=fl(_rs(37), 3, 5, 4, 3), phi_w=fl(_rs(38), 5), phi_b=fl(_rs(39), 1)),
       lambda ops, a: ops.cond_gate_pool(a["z"], a["phi_w"], a["phi_b"], 3, want_debug=True, want_plane_mean=True))
simple("linear", {"x": F, "weight": F, "bias": F}, lambda ops, d: dict(x=fl(_rs(40), 3, 6), weight=fl(_rs(41), 5, 6), bias=fl(_rs(42), 5)),
       lambda ops, a: ops.linear(a["x"], a["weight"], a["bias"]))
for _name, _mk, _fn in (("plane_mean", lambda ops, d: dict(x=fl(_rs(43), 3, 5, 4, 3)), lambda ops, a: ops.plane_mean(a["x"])),
                        ("plane_reduce", lambda ops, d: dict(x=fl(_rs(44), 3, 5, 4, 3)), lambda ops, a: ops.plane_reduce(a["x"], 1)),
                        ("plane_sum_sumsq", lambda ops, d: dict(x=fl(_rs(45), 3, 5, 4, 3)), lambda ops, a: ops.plane_sum_sumsq(a["x"])),
                        ("bicubic_plane_mean", lambda ops, d: dict(x=fl(_rs(46), 2, 3, 4, 5)), lambda ops, a: ops.bicubic_plane_mean(a["x"], (7, 9)))):
    simple(_name, {"x": F}, _mk, _fn)
simple("head_delta", {"head": F, "plane_means": F}, lambda ops, d: dict(head=fl(_rs(47), 3, 6), plane_means=fl(_rs(48), 3, 5)),
       lambda ops, a: ops.head_delta(a["head"], a["plane_means"]))

# ---- eval-loop memory policy
simple("confident_labels", {"probs": F, "join_label": I},
       lambda ops, d: dict(probs=torch.softmax(fl(_rs(49), 3, 35), 0), join_label=torch.from_numpy((np.arange(35) % 3 * (np.arange(35) % 5 == 0)).astype(np.int32))),
       lambda ops, a: ops.confident_labels(a["probs"], 0b111, a["join_label"], 0.5))
simple("label_onehot_nearest", {"label": I}, lambda ops, d: dict(label=torch.from_numpy((np.arange(63).reshape(7, 9) // 5 % 3).astype(np.int32))),
       lambda ops, a: ops.label_onehot_nearest(a["label"], 4, 5, 3))
simple("tta_merge", {"logits0": F, "logits1": F, "join_label": I},
       lambda ops, d: dict(logits0=fl(_rs(50), 3, 5, 7), logits1=fl(_rs(51), 3, 4, 6), join_label=torch.from_numpy((np.arange(35).reshape(5, 7) % 7 == 0).astype(np.int32))),
       lambda ops, a: ops.tta_merge([a["logits0"], a["logits1"]], [False, True], 5, 7, 0b111, a["join_label"], 0.5, "consistent", True),
       lambda r, a: [r["label"], r["entropy"], r["mean_probs"], r["label_flipped"]])


def _jf_call(ops, a):
    jf = ops.MaskJF(a["pred"].device)
    jf.add(a["pred"], a["gt"], 2)
    return jf


simple("MaskJF", {"pred": I, "gt": I},
       lambda ops, d: dict(pred=torch.from_numpy((np.arange(120).reshape(10, 12) // 7 % 3).astype(np.int32)), gt=torch.from_numpy((np.arange(120).reshape(10, 12) // 5 % 3).astype(np.int32))),
       _jf_call, lambda r, a: [r.accum])

# ---- decoder-side streams
GN_ROLES = {"x": F, "gamma": F, "beta": F, "residual": F, "out": OUT}


def _gn(seed, **more):
    rng = _rs(seed)
    return dict(x=fl(rng, 2, 8, 3, 5), gamma=fl(rng, 8), beta=fl(rng, 8), residual=fl(rng, 2, 8, 3, 5), out=blank("cpu", (2, 8, 3, 5)), **more)


simple("groupnorm_relu", GN_ROLES, lambda ops, d: _gn(52),
       lambda ops, a: ops.groupnorm_relu(a["x"], 4, a["gamma"], a["beta"], 1e-5, a["residual"], True, out=a["out"]))
simple("groupnorm_relu_scale", dict(GN_ROLES, head=F, weight=F, gate_bias=F),
       lambda ops, d: _gn(53, head=fl(_rs(54), 2, 6, scale=0.3), weight=fl(_rs(55), 8, 6, scale=0.3), gate_bias=fl(_rs(56), 8, scale=0.1)),
       lambda ops, a: ops.groupnorm_relu_scale(a["x"], 4, a["gamma"], a["beta"], 1e-5, a["residual"], True, a["head"], a["weight"], a["gate_bias"], out=a["out"]))
GCT_ROLES = {"plane_sums": F, "alpha": F, "gamma": F, "beta": F}
simple("gct_gate", GCT_ROLES, lambda ops, d: dict(plane_sums=fl(_rs(57), 3, 5).abs(), alpha=fl(_rs(58), 1, 5, 1, 1), gamma=fl(_rs(59), 1, 5, 1, 1), beta=fl(_rs(60), 1, 5, 1, 1)),
       lambda ops, a: ops.gct_gate(a["plane_sums"], a["alpha"], a["gamma"], a["beta"], 1e-5))
simple("gct_gate_multi", GCT_ROLES, lambda ops, d: dict(plane_sums=fl(_rs(61), 3, 5).abs(), alpha=fl(_rs(62), 2, 5), gamma=fl(_rs(63), 2, 5), beta=fl(_rs(64), 2, 5)),
       lambda ops, a: ops.gct_gate_multi(a["plane_sums"], a["alpha"], a["gamma"], a["beta"], 1e-5))
simple("channel_scale_multi", {"x": F, "gains": F, "out0": OUT, "out1": OUT},
       lambda ops, d: dict(x=fl(_rs(65), 3, 5, 4, 3), gains=fl(_rs(66), 2, 3, 5), out0=blank("cpu", (3, 5, 4, 3)), out1=blank("cpu", (3, 5, 4, 3))),
       lambda ops, a: ops.channel_scale_multi(a["x"], a["gains"], outs=[a["out0"], a["out1"]]))
simple("groupnorm_cat_relu", {"x0": F, "x1": F, "gamma": F, "beta": F, "tail": F, "out": OUT},
       lambda ops, d: dict(x0=fl(_rs(67), 2, 8, 3, 5), x1=fl(_rs(68), 2, 8, 3, 5), gamma=fl(_rs(69), 2, 8), beta=fl(_rs(70), 2, 8), tail=fl(_rs(71), 2, 3),
                           out=blank("cpu", (2, 19, 3, 5))),
       lambda ops, a: ops.groupnorm_cat_relu([a["x0"], a["x1"]], 4, a["gamma"], a["beta"], 1e-5, a["tail"], True, True, out=a["out"]))
simple("object_logit", {"x": F, "weight_bias": F}, lambda ops, d: dict(x=fl(_rs(72), 3, 5, 4, 3), weight_bias=fl(_rs(73), 3, 6)),
       lambda ops, a: ops.object_logit(a["x"], a["weight_bias"]))

# ---- the decoder's tail
simple("bicubic_cat_scale", {"x": F, "low": F, "gain": F, "out": OUT},
       lambda ops, d: dict(x=fl(_rs(74), 2, 3, 4, 5), low=fl(_rs(75), 2, 2, 7, 9), gain=fl(_rs(76), 2, 5), out=blank("cpu", (2, 5, 7, 9))),
       lambda ops, a: ops.bicubic_cat_scale(a["x"], a["low"], a["gain"], out=a["out"]))
simple("shortcut_stage", {"x": F, "low": F, "IA_head": F, "weight": F, "bias": F, "out": OUT},
       lambda ops, d: dict(x=fl(_rs(77), 2, 3, 4, 5), low=fl(_rs(78), 2, 2, 7, 9), IA_head=fl(_rs(79), 2, 6, scale=0.3), weight=fl(_rs(80), 5, 11, scale=0.3),
                           bias=fl(_rs(81), 5, scale=0.1), out=blank("cpu", (2, 5, 7, 9))),
       lambda ops, a: ops.shortcut_stage(a["x"], a["low"], a["IA_head"], a["weight"], a["bias"], want_debug=True, out=a["out"]))
simple("logit_head", {"x": F, "wb_fg": F, "wb_bg": F}, lambda ops, d: dict(x=fl(_rs(82), 3, 5, 4, 3), wb_fg=fl(_rs(83), 3, 6), wb_bg=fl(_rs(84), 3, 6)),
       lambda ops, a: ops.logit_head(a["x"], a["wb_fg"], a["wb_bg"]))
simple("background_merge", {"fg": F, "bg": F}, lambda ops, d: dict(fg=fl(_rs(85), 3, 1, 4, 3), bg=fl(_rs(86), 3, 1, 4, 3)),
       lambda ops, a: ops.background_merge(a["fg"], a["bg"]))
COND_N, COND_C, COND_D = 3, 24, 400        # test_cond_codes' first shape: (N, C, D) = (3, 24, 400)


def cond_codes_args(N, C, D, seed=87):
    """gap, plane_means, head and the six weights of aoc_cond_codes; b1 differs from the first row of W1 by far more than any rounding bound."""
    rng = _rs(seed)
    a = dict(gap=fl(rng, N, C), plane_means=fl(rng, N, C), head=fl(rng, N, D, scale=0.3), w1=fl(rng, C, C, scale=0.2), b1=fl(rng, C, scale=0.5) + 5.0,
             w2=fl(rng, C, C, scale=0.2), b2=fl(rng, C), w3=fl(rng, D, D, scale=0.05), b3=fl(rng, D))
    return a


COND_ROLES = {k: F for k in ("gap", "plane_means", "head", "w1", "b1", "w2", "b2", "w3", "b3")}
simple("cond_codes", COND_ROLES, lambda ops, d: cond_codes_args(3, 8, 12),
       lambda ops, a: ops.cond_codes(*[a[k] for k in COND_ROLES]))
PH_ROLES = {"feat": F, "weight": F, "bias": F, "gamma": F, "beta": F, "emb": F}
simple("prehead", PH_ROLES,
       lambda ops, d: dict(feat=fl(_rs(88), 2, 3, 4, 5), weight=fl(_rs(89), 8, 3, 1, 1), bias=fl(_rs(90), 8), gamma=fl(_rs(91), 8), beta=fl(_rs(92), 8), emb=fl(_rs(93), 4, 5, 6)),
       lambda ops, a: ops.prehead(a["feat"], a["weight"], a["bias"], 2, a["gamma"], a["beta"], 1e-5, a["emb"]))


# ---- the one-call paths: k-means chain, gates, frame
def _chain_args(ops, d):
    s = scene(ops, d)
    n_ad = POOL["O"] * 2 * POOL["kmax"]
    return dict(take(s, "pool", "init_rows", *PREP_FIELDS), table=blank("cpu", (n_ad, POOL["C"])), sqn=blank("cpu", (n_ad,)))


simple("cluster_chain", dict(PREP_ROLES, pool=F, init_rows=I, table=OUT, sqn=OUT), _chain_args,
       lambda ops, a: ops.cluster_chain(a["pool"], mk_prep(ops, a), [POOL["kmax"]], a["init_rows"], [a["table"]], [a["sqn"]]),
       lambda r, a: [a["table"], a["sqn"], r["centroids"], r["seg_offsets"]])


def _gates_args(ops, d):
    rng = _rs(94)
    N, c, D, H, W = 3, 4, 6, 4, 3
    a = dict(x0=fl(rng, N, c, H, W), x1=fl(rng, N, c, H, W), x2=fl(rng, N, c, H, W), head=fl(rng, N, D, scale=0.3),
             w0=fl(rng, c, D, scale=0.3), b0=fl(rng, c, scale=0.1), w1=fl(rng, c, D + c, scale=0.3), b1=fl(rng, c, scale=0.1),
             w2=fl(rng, c, 2 * c + D, scale=0.3), b2=fl(rng, c, scale=0.1), phi_w=fl(rng, c), phi_b=fl(rng, 1), cw1=fl(rng, c, c, scale=0.3), cb1=fl(rng, c),
             cw2=fl(rng, c, c, scale=0.3), cb2=fl(rng, c), cw3=fl(rng, D, D, scale=0.3), cb3=fl(rng, D))
    return a


def _gates_call(ops, a):
    entries = [(0, a["x0"], (a["w0"], a["b0"])), (1, a["x1"], (a["w1"], a["b1"])),
               (2, a["x2"], (a["w2"], a["b2"], a["phi_w"], a["phi_b"], a["cw1"], a["cb1"], a["cw2"], a["cb2"], a["cw3"], a["cb3"], 3))]
    batch = ops.GateBatch(entries, 3, 6)
    return batch(a["head"])


simple("GateBatch", {k: F for k in ("x0", "x1", "x2", "head", "w0", "b0", "w1", "b1", "w2", "b2", "phi_w", "phi_b", "cw1", "cb1", "cw2", "cb2", "cw3", "cb3")},
       _gates_args, _gates_call)


def _frame_args(ops, device, grate=1):
    """The `tiny` configuration (24 x 40 maps, 3 objects, C = 100): one pool frame, its label prep and proxy table, the frame after it."""
    import aoc_amd
    syn, hot = aoc_amd.synthetic, aoc_amd.hotpath
    cfg = syn.CONFIGS["tiny"]
    clip = syn.make_clip(cfg, 21, frames=2)
    O = cfg.n_obj
    emb = torch.from_numpy(clip["emb"]).to(device)
    lab = torch.from_numpy(np.stack([syn.one_hot(l, O) for l in clip["lab"]])).to(device)
    a = dict(ref_emb=emb[:1].contiguous(), ref_labels=lab[:1].contiguous(), prev_emb=emb[0].clone(), prev_labels=lab[0].clone(), cur_emb=emb[1].clone(),
             bias=torch.tensor([0.25, -0.5, 0.125], device=device))
    if grate > 1:
        return a
    mc = hot.MatchingConfig()
    n_rows = hot.proxy_table_rows(mc, O)
    if torch.device(device).type == "cuda":
        counts = [int(lab[0, ..., o].sum().item()) for o in range(O)]
        kmax = max(mc.cluster_levels)
        rows = np.zeros((len(mc.cluster_levels) * O, kmax), np.int32)
        for li, k in enumerate(mc.cluster_levels):
            for o, r in enumerate(syn.kmeans_init_rows(100 + li, counts, k)):
                if r is not None:
                    rows[li * O + o, :len(r)] = r
        ahead = hot.launch_cluster_proxies(mc, a["ref_emb"], a["ref_labels"], torch.from_numpy(rows).to(device))
        torch.cuda.synchronize()
        a.update({f: getattr(ahead.prep, f) for f in PREP_FIELDS}, table=ahead.table, sqn=ahead.sqn)
    else:
        a.update(_host_prep(syn.one_hot(clip["lab"][0], O).reshape(-1, O)), table=fl(_rs(95), n_rows, cfg.c), sqn=fl(_rs(96), n_rows).abs())
    return a


def _frame_call(ops, a):
    import aoc_amd
    cfg, mc = aoc_amd.synthetic.CONFIGS["tiny"], aoc_amd.hotpath.MatchingConfig()
    call = ops.FrameCall(cfg.h, cfg.w, cfg.c, cfg.n_obj, 2, mc.MODEL_MULTI_LOCAL_DISTANCE, mc.cluster_levels, mc.MODEL_MATCHING_BACKGROUND, mc.MODEL_EPSILON,
                         a["cur_emb"].device)
    call.reset()
    p = ops.LabelPrep()
    p.n, p.n_obj = cfg.h * cfg.w, cfg.n_obj
    for f in PREP_FIELDS:
        setattr(p, f, a[f])
    return call(a["ref_emb"], a["ref_labels"], a["prev_emb"], a["prev_labels"], a["cur_emb"], a["bias"], p, a["table"], a["sqn"], pool_key=1)


FRAME_F = ("ref_emb", "ref_labels", "prev_emb", "prev_labels", "cur_emb", "bias", "table", "sqn")
simple("FrameCall", dict(PREP_ROLES, **{k: F for k in FRAME_F}), _frame_args, _frame_call)


def _match_pool_call(ops, a):
    import aoc_amd
    cfg, mc = aoc_amd.synthetic.CONFIGS["tiny"], aoc_amd.hotpath.MatchingConfig()
    call = ops.FrameCall(cfg.h, cfg.w, cfg.c, cfg.n_obj, 2, mc.MODEL_MULTI_LOCAL_DISTANCE, mc.cluster_levels, mc.MODEL_MATCHING_BACKGROUND, mc.MODEL_EPSILON,
                         a["ref_emb"].device, global_atrous_rate=2)
    return call.match_pool(a["ref_emb"], a["ref_labels"])


simple("FrameCall.match_pool", {"ref_emb": F, "ref_labels": F}, lambda ops, d: {k: v for k, v in _frame_args(ops, d, 2).items() if k in ("ref_emb", "ref_labels")},
       _match_pool_call, covers=["FrameCall"])
