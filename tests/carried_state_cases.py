"""Cases for what the matching entries keep between calls and for how they size persistent grids.  Shared by test_carried_state_host.py (no
GPU) and test_gpu_carried_state.py.  Pure numpy; the library is not imported here.  No bound is defined here: every reference and every
bound is global_match_bounds' (split_dense_ref for a frame the split kernels answer, dense_ref for one the exact-fp32 kernels take over).

1. Sequences for aoc_dense_match_min_split_cached.  A sequence is a list of steps in ONE workspace; a step names a pool state, whether the
   call builds the plan (reuse_plan = 0) or reuses it, its query and what must answer it:
     "split"     the split kernels (the float64 bound of split_dense_ref; the prune counters move),
     "takeover"  the exact-fp32 kernels inside the same call (dense_ref's bound, bit-equal to aoc_dense_match_min, counters stay zero),
     "empty"     n_fg = 0: 1.0 transformed, +inf raw.
   A pool state is dense_inputs of a DenseCase (one-hot, or takeover_soft's soft rows) with the labels rebuilt from an owner array where a
   sequence needs another object absent or the seed structure.  "n" in the sequence names counts kept rows as in DenseCase.n_fg: 400 kept
   rows are 450 pool rows, which is >= m = 150, so dense_seed_kernel runs; 133 kept rows are 149 = m - 1 pool rows, where it does not.
   Every frame has its own query: fresh draws with the same planted structure as dense_inputs (a near copy of each planted kept row at
   distance PLANT_LEN k, k >= 2 all different, and of the unkept trap row at k = 1 in the last pixel), so every slip of split_dense_slips
   shows at every frame and a frame answered with another frame's output leaves the bound almost everywhere.
2. split_nsplit of dense_split.hip restated, and the (m, budget) pairs of the CU-budget sweep.
3. The proxy-correlation shapes of the sweep: item tiles per frame against the grid at budget 1."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import global_match_bounds as gb
from global_match_bounds import DenseCase, PLANT_LEN, f32

# the three helpers of global_match_bounds that carry a leading underscore there, bound once: a rename shows here and nowhere else
unit_vector, proxy_case, reference_bundle = gb._unit, gb._pcase, gb._bundle

M = 150
BUDGETS = (0, 1, 2, 3, 7, 64, 255, 257, 1024)
STALE_SHARE = 0.75          # of a frame's outputs leave its bound when the frame before, or another pool state, answers it (host test)


# ------------------------------------------------------------------------------------------ pool states
def owner_of(inp, n_obj):
    """The object each pool row is right for in a one-hot state, from the rows' wrong bits (every row has them, kept or not)."""
    mask = (1 << n_obj) - 1
    free = ~inp["wrong"].astype(np.int64) & mask
    assert all(bin(v).count("1") == 1 for v in free), "not one-hot"
    return np.log2(free).astype(np.int64)


def relabel(inp, owner, n_obj):
    """inp with right / wrong bits, counts, obj_rows and obj_offsets rebuilt for `owner`, as dense_inputs builds them (the bits from n_obj up
    stay; the packed lists are padded with the trap row)."""
    n_pool = inp["pool"].shape[0]
    is_kept = (inp["right"].astype(np.int64) >> 31) & 1 == 1
    all_obj = (1 << n_obj) - 1
    trap = int(inp["fg_rows"][-1])
    wrong = (inp["wrong"].astype(np.int64) & ~all_obj & 0xFFFFFFFF) | (all_obj & ~(1 << owner))
    right = np.where(is_kept, (1 << 31) | (1 << owner), 0)
    counts = np.zeros(n_obj + 1, np.int32)
    obj_rows = np.full(n_obj * n_pool, trap, np.int32)
    offsets = np.zeros(n_obj + 1, np.int32)
    for o in range(n_obj):
        rows_o = np.nonzero(is_kept & (owner == o))[0]
        counts[o] = rows_o.size
        obj_rows[offsets[o]:offsets[o] + rows_o.size] = rows_o
        offsets[o + 1] = offsets[o] + rows_o.size
    counts[n_obj] = inp["n_fg"]
    out = dict(inp)
    out.update(wrong=wrong.astype(np.uint32), right=right.astype(np.uint32), counts=counts, obj_rows=obj_rows, obj_offsets=offsets)
    return out


StateSpec = namedtuple("StateSpec", "case absent seeded soft")


def _state(name, C=100, n_fg=400, n_obj=5, layout="planes", absent=None, seeded=False, soft=False, m=M):
    return StateSpec(DenseCase(name, C, m, n_fg, n_obj, False, layout), absent, seeded, soft)


STATES = {s.case.name: s for s in [
    _state("cs_O3", n_obj=3),
    _state("cs_O16", n_obj=16, layout="pixels"),
    _state("cs_absent3"),                                   # dense_inputs leaves object 3 of five without a row
    _state("cs_absent0", absent=0, layout="pixels"),
    _state("cs_absent4", absent=4),
    _state("cs_seeded", seeded=True, layout="pixels"),      # 450 pool rows >= m
    _state("cs_unseeded", n_fg=133, seeded=True),           # 149 pool rows = m - 1
    _state("cs_mid"),
    _state("cs_soft", soft=True),
    _state("cs_empty", n_fg=0, layout="pixels"),
    _state("cs_A"),
    _state("cs_B", n_fg=330, n_obj=3, layout="pixels"),
    _state("cs_C36", C=36),
    _state("cs_C4", C=4, n_obj=3, layout="pixels"),
]}
SEED_OBJECT = 1         # the object whose only row among the last m pool rows is SEED_LONE's; every other row of it is older


@functools.lru_cache(maxsize=None)
def state_inputs(name):
    """dense_inputs of the state, relabelled where the state asks for it.  Seeded states also get `seed`: dict(lone = the one row of
    SEED_OBJECT among the last m pool rows, exact = (query pixel, pool row) of the pixel every frame copies from its seed row)."""
    spec = STATES[name]
    case = spec.case
    if spec.soft:
        inp = gb.dense_takeover_inputs(gb.DENSE_TAKEOVER_BY_NAME["takeover_soft"])
        assert (case.C, case.m, case.n_fg, case.n_obj) == (100, M, 400, 5)
        return inp
    inp = gb.dense_inputs(case, onehot=True)
    if case.n_fg == 0:
        return inp
    owner = owner_of(inp, case.n_obj)
    if spec.absent is not None:         # swap the absent object 3 with the wanted one
        a, b = spec.absent, gb.absent_object(case.n_obj)
        owner = np.where(owner == a, b, np.where(owner == b, a, owner))
        inp = relabel(inp, owner, case.n_obj)
        inp["bias"] = inp["bias"].copy()
    if spec.seeded:
        n, m = inp["pool"].shape[0], case.m
        is_kept = (inp["right"].astype(np.int64) >> 31) & 1 == 1
        last = np.arange(max(0, n - m), n)
        mine = last[is_kept[last] & (owner[last] == SEED_OBJECT)]
        lone = int(mine[0])
        owner = owner.copy()
        owner[mine[1:]] = 0
        unkept_last = last[~is_kept[last]]
        owner[unkept_last] = np.where(owner[unkept_last] == SEED_OBJECT, 0, owner[unkept_last])
        inp = relabel(inp, owner, case.n_obj)
        # the exact pixel: a kept row of the last m whose pixel no plant uses (plants sit in pixels below 40 and in the last one)
        cand = [int(j) for j in last if is_kept[j] and j != lone and 40 <= j - (n - m) <= m - 2 and j != inp["fg_rows"][-1]]
        inp["seed"] = dict(lone=lone, exact=(cand[0] - (n - m), cand[0]))
    return inp


def frame_query(state, frame, seq, hot=False):
    """The query of one frame of sequence `seq` against pool state `state`.  hot: one value of 80.0 (80 x 2^10 > 65000 and 80^2 > 4000)."""
    spec = STATES[state]
    case = spec.case
    inp = state_inputs(state)
    C, m = case.C, case.m
    rng = np.random.RandomState(zlib.crc32(f"{seq}/{state}/{frame}".encode()) & 0x7FFFFFFF)
    q = (0.5 / np.sqrt(C) * rng.standard_normal((m, C))).astype(f32)
    kept = inp["fg_rows"][:case.n_fg]
    for t, p in enumerate(inp["planted"]):
        i = (t + 3 * frame) % m
        assert i < 40 <= m - 2
        q[i] = (inp["pool"][kept[p]].astype(np.float64) + PLANT_LEN * (2 + t) * unit_vector(rng, C)).astype(f32)
    if case.n_fg:
        q[m - 1] = (inp["pool"][inp["fg_rows"][-1]].astype(np.float64) + PLANT_LEN * unit_vector(rng, C)).astype(f32)
    if "seed" in inp:
        i, j = inp["seed"]["exact"]
        q[i] = inp["pool"][j]
    if hot:
        q[100, 7] = 80.0
    return q


# ------------------------------------------------------------------------------------------ sequences
Step = namedtuple("Step", "state reuse frame expect hot same zero_flag")


def _steps(state, n_reuse, first=0, expect="split"):
    return [Step(state, int(k > 0), first + k, expect, False, False, False) for k in range(n_reuse + 1)]


def _seeded(state):
    s = _steps(state, 3)
    s[2] = s[2]._replace(same=True)                        # frame 2 is frame 1 again
    return s


def _mid():
    s = _steps("cs_mid", 1)
    s.append(Step("cs_mid", 1, 2, "takeover", True, False, False))
    s += [Step("cs_mid", 1, f, "takeover", False, False, False) for f in (3, 4)]     # ordinary queries, the flag still raised
    s.append(Step("cs_mid", 1, 5, "takeover", False, False, True))                   # the flag zeroed: the gate in the workspace stays set
    s.append(Step("cs_mid", 0, 6, "split", False, False, True))                      # the flag zero, the plan rebuilt
    s += [Step("cs_mid", 1, f, "split", False, False, False) for f in (7, 8)]
    return s


SEQUENCES = {
    "plain_O3": _steps("cs_O3", 4),
    "plain_O16": _steps("cs_O16", 4),
    "absent_3": _steps("cs_absent3", 3),
    "absent_first": _steps("cs_absent0", 3),
    "absent_last": _steps("cs_absent4", 3),
    "seeded": _seeded("cs_seeded"),
    "unseeded": _seeded("cs_unseeded"),
    "takeover_mid": _mid(),
    "soft_gate": _steps("cs_soft", 3, expect="takeover"),
    "no_rows": _steps("cs_empty", 2, expect="empty"),
    "A_then_B": _steps("cs_A", 2) + _steps("cs_B", 2, first=3),
    "B_then_A": _steps("cs_B", 2) + _steps("cs_A", 2, first=3),
    "C36": _steps("cs_C36", 4),
    "C4": _steps("cs_C4", 4),
}
BOTH_RECORD_ORDERS = ("plain_O3", "plain_O16")      # run with row-major and with tiled query records; every other sequence with tiled ones


def step_query(seq, k):
    """The query of step k of a sequence (a `same` step repeats the one before)."""
    step = SEQUENCES[seq][k]
    if step.same:
        return step_query(seq, k - 1)
    return frame_query(step.state, step.frame, seq, step.hot)


def _frame_ref(state, query, expect, with_slips=True):
    spec = STATES[state]
    case = spec.case
    inp = state_inputs(state)
    args = (query, inp["pool"], inp["fg_rows"][:case.n_fg], inp["wrong"], case.n_obj)
    if expect == "empty":
        want = np.full((case.n_obj, case.m), np.inf)
        return dict(raw=(want, np.zeros_like(want), {}), transformed=(np.ones_like(want), np.zeros_like(want), {}))
    ref, kinds = (gb.split_dense_ref, gb.split_dense_slips(case)) if expect == "split" else (gb.dense_ref, gb.dense_slips(case))
    want, tol = ref(*args)
    slips = {k: ref(*args, slip=k, planted=inp["planted"])[0] for k in kinds} if with_slips else {}
    want_t, tol_t = gb.transform_ref(want, tol, inp["bias"])
    t_slips = {k: gb.transform_ref(v, np.zeros_like(tol), inp["bias"])[0] for k, v in slips.items() if k != "wrong_excluded"}
    for a in (want, tol, want_t, tol_t, *slips.values(), *t_slips.values()):
        a.setflags(write=False)
    return dict(raw=(want, tol, slips), transformed=(want_t, tol_t, t_slips))


@functools.lru_cache(maxsize=None)
def step_ref(seq, k):
    """-> dict(raw=(want, tol, slips), transformed=(want, tol, slips)) of step k, computed once, read-only."""
    step = SEQUENCES[seq][k]
    if step.same:
        return step_ref(seq, k - 1)
    return _frame_ref(step.state, step_query(seq, k), step.expect)


def other_state_ref(state_q, state_pool, query):
    """The float64 answer (raw, transformed) for `query` from the rows and labels of another pool state: what a call would give that went on
    with the plan of the state before."""
    r = _frame_ref(state_pool, query, "split", with_slips=False)
    return r["raw"][0], r["transformed"][0]


def sequence_workspace_states(seq):
    return sorted({s.state for s in SEQUENCES[seq]})


# ------------------------------------------------------------------------------------------ the CU budget: dense
def split_nsplit(m, budget):
    """split_nsplit of dense_split.hip in the product's configuration (eight waves of two 32-pixel query tiles: 512 query pixels per row
    block; one workgroup per CU; at most two rounds; 64 splits at most), in the same double arithmetic.  budget 0 = 256 CUs."""
    row_blocks = (m + 511) // 512
    n_cu = budget if budget > 0 else 256
    best, best_eff = 1, 0.0
    for k in (1, 2):
        ns = min(64, max(1, (n_cu * k) // row_blocks))
        blocks = row_blocks * ns
        rounds = (blocks + n_cu - 1) // n_cu
        eff = blocks / (float(n_cu) * rounds)
        if eff >= best_eff - 0.005:
            best_eff = max(eff, best_eff)
            best = ns
    return best


def plan_tiles(counts, n_obj):
    """split_plan_kernel: object-pure tiles of 32 rows."""
    return int(sum((int(c) + 31) // 32 for c in counts[:n_obj]))


BUDGET_M = (150, 513, 1100)                                  # 1, 2 and 3 row blocks
BUDGET_POOLS = {"small": (40, 3), "large": (2100, 5)}        # (kept rows, objects): 3 tiles and more than 64


def budget_case(m, pool):
    n_fg, n_obj = BUDGET_POOLS[pool]
    return DenseCase(f"cs_budget_m{m}_{pool}", 100, m, n_fg, n_obj, False, "planes" if m != 513 else "pixels")


for _m in BUDGET_M:
    for _p in BUDGET_POOLS:
        STATES[budget_case(_m, _p).name] = StateSpec(budget_case(_m, _p), None, False, False)
        SEQUENCES[budget_case(_m, _p).name] = _steps(budget_case(_m, _p).name, 1)


# ------------------------------------------------------------------------------------------ the CU budget: proxy correlation
# item tiles per frame T = ceil(m / 32); at budget 1 the batched kernel runs 1 workgroup and the records kernels 2
CORR_SHAPES = [(33, 1), (65, 1), (97, 1), (33, 3), (650, 1), (650, 3)]        # (m, frames)


def corr_items(m, frames):
    return (m + 31) // 32 * frames


def corr_case(m):
    """The general structure (sets of 0 .. 33 proxies, runs of single-proxy sets: 16 + 16 + 1 and more) at m query pixels."""
    return proxy_case(f"cs_corr_m{m}", 100, m)


def corr_ref(m, frame, records):
    case = corr_case(m)
    inp = gb.proxy_inputs(case, frame)
    ref = functools.partial(gb.split_proxy_ref, inp["query"], inp["proxies"], inp["sqnorm"], inp["set_begin"], inp["set_size"], records)
    return reference_bundle(ref, gb.cb_transform_ref, gb.split_slips(case), gb.split_slips(case, transformed=True), inp["bias"])


LEVEL_CASES = {"levels_8_16_32_O6": ([8, 16, 32], 6), "levels_64_O24": ([64], 24)}      # several passes; more passes than one table array holds
LEVEL_SLIPS = ["past_the_end", "tail_channels", "two_products", "one_product", "norm_one_piece"]
CORR_MAX_TILES, CORR_MAX_OUT, CORR_MAX_PASSES = 5, 64, 16      # AOC_CORR_MAX_TILES, AOC_CORR_MAX_OUT, CB_MAX_PASSES


def corr_passes(set_begin, set_size, set_off, max_tiles=CORR_MAX_TILES):
    """cb_run's packing loop of correlation_batched.hip restated -> the 32-row proxy tiles of every pass (launch).  Class by class:
    single-proxy sets over consecutive proxies with a constant output step share one column-wise tile of up to 32, and a pass takes one such
    tile, as its first; sets of up to 8 proxies go four to a tile, sets of up to 16 two to a tile (a tile holds one class); a larger set
    (and an empty one counts as 8 or fewer) takes ceil(size / 32) tiles of its own.  A pass holds max_tiles tiles and CORR_MAX_OUT sets."""
    begin, size, off = ([int(v) for v in a] for a in (set_begin, set_size, set_off))
    cls_of = lambda n: 0 if n == 1 else 1 if n <= 8 else 2 if n <= 16 else 3
    passes = []
    st = dict(n=0, n_out=0)

    def flush():
        if st["n"]:
            passes.append(st["n"])
        st.update(n=0, n_out=0)

    for cls in range(4):
        is_open, groups, t_begin, t_cnt, t_step, last_off = False, 0, 0, 0, 0, 0
        for s in range(len(size)):
            if cls_of(size[s]) != cls:
                continue
            if cls == 0:
                cont = is_open and t_cnt < 32 and begin[s] == t_begin + t_cnt
                if cont:
                    step = off[s] - last_off
                    if t_cnt == 1:
                        t_step = step
                    elif t_step != step:
                        cont = False
                if not cont or st["n_out"] + 1 > CORR_MAX_OUT:
                    if st["n"] > 0:
                        flush()
                    is_open, t_begin, t_cnt = True, begin[s], 0
                    st["n"] += 1
                st["n_out"] += 1
                last_off, t_cnt = off[s], t_cnt + 1
            elif cls in (1, 2):
                if not is_open or groups + cls > 4 or st["n_out"] + 1 > CORR_MAX_OUT:
                    if st["n"] + 1 > max_tiles or st["n_out"] + 1 > CORR_MAX_OUT:
                        flush()
                    is_open, groups = True, 0
                    st["n"] += 1
                st["n_out"] += 1
                groups += cls
            else:
                nt = (size[s] + 31) // 32
                if st["n"] + nt > max_tiles or st["n_out"] + 1 > CORR_MAX_OUT:
                    flush()
                st["n_out"] += 1
                st["n"] += nt
                is_open = False
    flush()
    return passes


def levels_inputs(name, m, frame=0):
    """The proxy table of a cluster frame, as aoc_frame_enqueue lays it out: per level, per object TWO sets of `level` proxies (the
    foreground and the background code book), level-major, then one single-proxy set per object (the k = 1 rows), and one proxy past the
    last set.  proxy_inputs' dict.  The first proxy of every set but the first is a near copy of query s mod m (at PLANT_LEN (1 + s)): the
    set before must not take it."""
    levels, n_obj = LEVEL_CASES[name]
    sizes = np.asarray([k for k in levels for _ in range(2 * n_obj)] + [1] * n_obj, np.int32)
    begin = (np.cumsum(sizes) - sizes).astype(np.int32)
    n_set, n_proxy, C = sizes.size, int(sizes.sum()) + 1, 100
    rng = np.random.RandomState(zlib.crc32(f"{name}/{m}/{frame}".encode()) & 0x7FFFFFFF)
    s = 0.5 / np.sqrt(C)
    query = (s * rng.standard_normal((m, C))).astype(f32)
    proxies = (s * rng.standard_normal((n_proxy, C))).astype(f32)
    for t in range(1, n_set):
        proxies[begin[t]] = (query[t % m].astype(np.float64) + PLANT_LEN * (1 + t) * unit_vector(rng, C)).astype(f32)
    sqnorm = (proxies * proxies).sum(1, dtype=f32)
    bias = (rng.uniform(0.25, 1.0, n_set) * np.where(np.arange(n_set) % 2 == 0, 1.0, -1.0)).astype(f32)
    set_off = np.arange(n_set, dtype=np.int64) * (m + 3) + 2
    named = set_off[:, None] + np.arange(m)[None, :]
    return dict(query=query, proxies=proxies, sqnorm=sqnorm, bias=bias, set_begin=begin, set_size=sizes, set_off=set_off, stride=1,
                out_len=n_set * (m + 3) + 7, named=named)


def levels_ref(name, m, frame=0):
    inp = levels_inputs(name, m, frame)
    ref = functools.partial(gb.split_proxy_ref, inp["query"], inp["proxies"], inp["sqnorm"], inp["set_begin"], inp["set_size"], True)
    return reference_bundle(ref, gb.cb_transform_ref, LEVEL_SLIPS, LEVEL_SLIPS + ["other_bias"], inp["bias"])


def corr_takeover_inputs(m=97):
    """The general structure with one query value of 80.0 (no plant copies the last query): the exact-fp32 kernel recomputes the launch."""
    inp = gb.proxy_inputs(corr_case(m))
    inp["query"][m - 1, 7] = 80.0
    return inp


def corr_takeover_ref(m=97):
    case = corr_case(m)
    inp = corr_takeover_inputs(m)
    ref = functools.partial(gb.proxy_ref, inp["query"], inp["proxies"], inp["sqnorm"], inp["set_begin"], inp["set_size"])
    return reference_bundle(ref, gb.transform_ref, gb.proxy_slips(case), gb.proxy_slips(case, transformed=True), inp["bias"])
