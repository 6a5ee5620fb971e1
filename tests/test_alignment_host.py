"""The pointer-alignment contract on the host: no GPU, no library.

Three things are held here (tests/alignment_cases.py has the table, include/aoc_hip.h "Pointer alignment" the text):
  * the table against the header: every pointer parameter of every covered entry's prototype (and every data pointer of the descriptors)
    has a class, the header's own list of class-16 pointers says the same, every class-16 pointer names the source line that decides it;
  * aoc_amd.ops against the table: every registry case of tests/ops_contract_cases.py that reaches a covered entry runs with each tensor
    4 / 8 / 12 bytes off the 16-byte grid, one at a time and all inputs at once, under a stub library that decodes every argument (the
    descriptors included) into (entry, parameter, address); the stub, the rule and the variants live beside the table.  A class-16 position then receives a live, contiguous tensor of the canonical
    dtype and size ON the grid -- or the call raised before the library was entered, which it must for a caller-provided output; a class-4
    position receives the caller's own storage (no silent copy, of an output least of all);
  * the helper itself (ops._a16)."""
import os

import pytest
import torch

from aoc_amd import ops

import alignment_cases as ac
import ops_contract_cases as occ

HEADER, PARAMS = ac.HEADER, ac.PARAMS
COVERING = ac.covering()

# what the alignment contract was asked to cover (the issue's list, spelled out)
ENTRIES = """aoc_label_prep aoc_label_bits aoc_kmeans_segmented aoc_kmeans_segmented_ex aoc_kmeans_segmented_rep aoc_kmeans_replicate
aoc_kmeans_replicate_levels aoc_build_proxies aoc_proxy_corr_min aoc_proxy_corr_min_f16 aoc_proxy_corr_min_batched aoc_proxy_corr_min_records
aoc_proxy_corr_min_records_cached aoc_dense_match_min aoc_dense_match_min_f16 aoc_dense_match_argmin aoc_split_rows aoc_split_rows_tiled
aoc_dense_match_min_split aoc_dense_match_min_split_cached aoc_dense_match_grad aoc_proxy_match_grad aoc_local_window_match
aoc_local_window_match_ex aoc_local_window_match_pair aoc_local_window_match_argmin aoc_local_match_grad aoc_local_prep aoc_resize_bilinear_hwc
aoc_resize_bilinear_hwc_ex aoc_resize_nearest_bits aoc_atrous_subsample aoc_proxy_set_match_argmin aoc_proxy_set_match_grad aoc_centroid_avg_grad
aoc_proto_finish aoc_fg2bg_min aoc_frame_enqueue aoc_cluster_chain_enqueue""".split()

# entries aoc_amd.ops never calls by that name: it calls the general form, which the named one forwards to inside the library
NOT_CALLED_BY_OPS = {
    "aoc_kmeans_segmented": "forwards to aoc_kmeans_segmented_rep (pool_rows = 0, n_rep = 1)", "aoc_kmeans_segmented_ex": "forwards to aoc_kmeans_segmented_rep (n_rep = 1)",
    "aoc_local_window_match": "forwards to aoc_local_window_match_ex", "aoc_resize_bilinear_hwc": "forwards to aoc_resize_bilinear_hwc_ex",
    "aoc_dense_match_min_split_cached": "called by aoc_frame_enqueue inside the library; ops calls aoc_dense_match_min_split, which forwards to it",
    "aoc_proxy_corr_min_f16": "the float16=True form of ops.proxy_corr_min: same wrapper, same pointers (no registry case takes the switch)",
    "aoc_dense_match_min_f16": "the float16=True form of ops.dense_match_min: same wrapper, same pointers (no registry case takes the switch)",
}


# ------------------------------------------------------------------------------------------ the table against the header
def test_the_covered_entries_are_the_ones_asked_for():
    assert set(ac.covered_entries()) == set(ENTRIES)
    assert set(ENTRIES) <= set(PARAMS), "a covered entry has no prototype in the header"


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_pointer_parameter_has_a_class(entry):
    want = ac.prototype_pointers(HEADER)[entry]
    assert list(ac.CLASS[entry]) == want or set(ac.CLASS[entry]) == set(want), f"{entry}: the header has {want}, the table {list(ac.CLASS[entry])}"
    assert set(ac.CLASS[entry].values()) <= {4, 16}
    for p, cls in ac.CLASS[entry].items():
        assert ((entry, p) in ac.WHY) == (cls == 16), f"{entry}.{p}: class {cls} and {'a' if (entry, p) in ac.WHY else 'no'} deciding line"
        if p in ac.HOST:
            assert cls == 4, f"{entry}.{p} is a host pointer"


@pytest.mark.parametrize("struct", ac.STRUCTS)
def test_every_descriptor_pointer_has_a_class(struct):
    members = [m for m in ac.struct_pointers(HEADER, struct) if m not in ac.NOT_DATA.get(struct, ())]
    assert set(members) == set(ac.CLASS[struct]), f"{struct}: the header has {members}"
    for p, cls in ac.CLASS[struct].items():
        assert ((struct, p) in ac.WHY) == (cls == 16)
    assert struct in ac.DESCRIPTORS.values()


def test_the_header_states_the_same_classes():
    """The header's list "Class-16 pointers per entry" against the table, both ways."""
    import re
    section = HEADER[HEADER.index("Pointer alignment"):HEADER.index("#ifndef AOC_HIP_H")]
    stated = {}
    for line in section.splitlines():
        m = re.match(r"^ \*\s+((?:aoc_\w+)(?:\s*/\s*aoc_\w+)*)\s+16:\s*(.*)$", line)
        if m:
            names = set() if m.group(2).strip() == "-" else {p.strip() for p in m.group(2).split(",")}
            for e in m.group(1).split("/"):
                assert e.strip() not in stated, f"{e.strip()} listed twice"
                stated[e.strip()] = names
    assert set(stated) == set(ac.CLASS), f"header and table name different entries: {sorted(set(stated) ^ set(ac.CLASS))}"
    for e, names in stated.items():
        assert names == {p for p, c in ac.CLASS[e].items() if c == 16}, e
    for e in ac.CONDITIONAL:
        assert e in section
    assert "X % 4 == 0" in section and "tables_key != NULL" in section
    # ... and every covered prototype / descriptor carries its own line of that list right above it
    for e, names in stated.items():
        head = ("typedef struct " + e + " {") if e in ac.STRUCTS else ("int " + e + "(")
        at = HEADER.index("\n" + head)
        line = HEADER[:at].rsplit("\n", 1)[1]
        m = re.match(r'/\* Alignment \("Pointer alignment" above\): class 16: ([^;]*); every other pointer class 4\. \*/$', line)
        assert m, f"{e}: no alignment line above its prototype, but {line!r}"
        assert ({p.strip() for p in m.group(1).split(",")} - {"-"}) == names, e


def test_deciding_lines_name_wide_accesses():
    """Every `file.hip:line` a class-16 pointer names as its FIRST reference holds a 16-byte access -- or, for the descriptor and workspace
    pointers of the frame and chain calls, the function the WHY text names (an entry that takes the pointer as a class-16 parameter, or the
    carve of the workspace).  That the pointer is the argument in the class-16 POSITION of that call is read by eye, not by this test."""
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robust-video-object-segmentation_amd", "csrc")
    wide = re.compile(r"float4|uint4|u32x4|global_load_lds_dwordx4|raw_buffer_load_b128|glds16|AocCorrTiles")
    for key, why in ac.WHY.items():
        m = re.search(r"(\w+\.hip):(\d+)", why)
        assert m, f"{key}: no source line in {why!r}"
        lines = open(os.path.join(root, m.group(1))).read().splitlines()
        text = lines[int(m.group(2)) - 1]
        named = [f for f in re.findall(r"\b(aoc_\w+|\w+_carve)\b", why) if f + "(" in text]
        assert wide.search(text) or named, f"{key}: {m.group(1)}:{m.group(2)} reads {text.strip()!r}"
        if named and not wide.search(text):
            assert any(f in ac.CLASS and 16 in ac.CLASS[f].values() for f in named) or any(f.endswith("_carve") for f in named), (key, named)


# ------------------------------------------------------------------------------------------ ops against the table
def test_every_covered_entry_is_reached_by_a_registry_case():
    reached = {e for n in COVERING for e, _, _ in ac.canonical(n)[3].seen}
    missing = set(ENTRIES) - reached
    assert missing == set(NOT_CALLED_BY_OPS), f"covered entries no registry case reaches: {sorted(missing)}; expected {sorted(NOT_CALLED_BY_OPS)}"
    assert set(ac.STRUCTS) <= reached, "a descriptor no registry case fills"


@pytest.mark.parametrize("name", COVERING)
def test_alignment_on_the_host(name):
    case, canon_a, canon_rec, canon_stub = ac.canonical(name)
    for n in ac.tensors(case, canon_a):
        assert canon_a[n].data_ptr() % 16 == 0, f"{name}: the canonical `{n}` is not on the grid"
    for e, p, addr in canon_stub.seen:
        assert ac.CLASS[e][p] == 4 or addr is None or addr % 16 == 0, f"{name}: the canonical call hands {e}.{p} an address off the grid"
    failed, n_run = [], 0
    for label, moved, k in ac.variants(case, canon_a):
        a = dict(case.build(ops, "cpu"))
        for n in moved:
            a[n] = ac.off_grid(a[n], k)[0]
        err, rec, stub = ac.run(case, a)
        n_run += 1
        bad = ac.check_variant(case, canon_a, canon_stub, canon_rec, a, moved, err, rec, stub)
        if bad:
            failed.append(f"({name}, {label}): " + "; ".join(bad))
    assert n_run, f"{name}: no variant was run"
    assert not failed, "\n".join(failed)


def test_cases_with_class16_inputs_exist():
    with16 = [n for n in COVERING if ac.class16_inputs(n)]
    assert len(with16) >= 15, with16


# ------------------------------------------------------------------------------------------ the helper
def test_a16():
    t = torch.arange(12, dtype=torch.float32)
    assert t.data_ptr() % 16 == 0
    assert ops._a16("x", t) is t and ops._a16("x", t, output=True) is t and ops._a16("x", None) is None
    for k in ac.OFFSETS:
        v, buf, lo = ac.off_grid(t, k)
        c = ops._a16("x", v)
        assert c is not v and c.data_ptr() % 16 == 0 and c.is_contiguous() and c.dtype == v.dtype and torch.equal(c, v)
        with pytest.raises(ValueError):
            ops._a16("x", v, output=True)
