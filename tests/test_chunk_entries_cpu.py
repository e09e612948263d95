"""The five chunk-attention wrappers of the ctypes binding put every argument where include/speckv_ext.h declares it, without a GPU
and without a library: SpeckvLib.attend_chunk* are called on an instance whose `_ext` only records, every argument a value of its
own, and what `_ext` received is compared with the header's declaration -- the parameter names, their order and which of them are
pointers come from the header, never from the binding.  A wrapper takes the header's parameters in the header's order without the
leading n_seq, which it derives from `handles`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cxl_speckv_amd import speckv_ctypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
ENTRIES = {"speckv_ext_attend_chunk": "attend_chunk", "speckv_ext_attend_chunk_masked": "attend_chunk_masked",
           "speckv_ext_attend_chunk_split": "attend_chunk_split", "speckv_ext_attend_chunk_window": "attend_chunk_window",
           "speckv_ext_attend_chunk_tree_window": "attend_chunk_tree_window"}
PER_SEQ = {"handles": (C.c_uint64, np.uint64), "pos_end": (C.c_uint32, np.uint32), "n_q": (C.c_uint32, np.uint32),
           "tail_idx": (C.c_int32, np.int32)}
NULLABLE = ("tail_idx", "d_lse", "d_k_tail", "d_mask")


def declared(entry):
    """[(name, is a pointer)] of the entry's parameters, in the header's order"""
    text = re.search(entry + r"\s*\((.*?)\);", HEADER[HEADER.index("speckv_status_t " + entry + "("):], re.S).group(1)
    return [(p.split()[-1].lstrip("*"), "*" in p) for p in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]


def sentinels(entry):
    """a value of its own per declared parameter: three-element lists per sequence, a float for sm_scale, small distinct ints"""
    values = {}
    for k, (name, _) in enumerate(declared(entry)):
        values[name] = [100 * k + 1, 100 * k + 2, 100 * k + 3] if name in PER_SEQ else 0.375 if name == "sm_scale" else 1000 + k
    values["n_seq"] = 3
    return values


def call(entry, values):
    """the wrapper called positionally with `values` in the header's order (n_seq left out); what _ext received"""
    lib, got = speckv_ctypes.SpeckvLib.__new__(speckv_ctypes.SpeckvLib), []
    lib._ext = lambda name, *args: got.append((name, args))
    getattr(lib, ENTRIES[entry])(*[values[name] for name, _ in declared(entry) if name != "n_seq"])
    assert len(got) == 1 and got[0][0] == entry
    assert len(got[0][1]) == len(declared(entry)) == len(speckv_ctypes._EXT_SIGNATURES[entry])
    return dict(zip([name for name, _ in declared(entry)], got[0][1]))


def check_plain(entry, values, got, skip=()):
    """scalars by value, pointers as c_void_p by .value"""
    assert got["n_seq"] == 3
    for name, pointer in declared(entry):
        if name in PER_SEQ or name in skip:
            continue
        if pointer:
            assert isinstance(got[name], C.c_void_p) and got[name].value == values[name], name
        else:
            assert got[name] == values[name], name


def test_the_header_declares_what_this_test_assumes():
    base = [name for name, _ in declared("speckv_ext_attend_chunk")]
    assert base[0] == "n_seq" and len(base) == 20 and set(PER_SEQ) <= set(base) and "sm_scale" in base
    assert [p for _, p in declared("speckv_ext_attend_chunk")].count(True) == 12
    for entry in ENTRIES:
        names = [name for name, _ in declared(entry)]
        assert len(set(names)) == len(names) and names[:16] == base[:16] and names[-4:] == base[-4:], entry
    assert [name for name, _ in declared("speckv_ext_attend_chunk_tree_window")][16:21] == ["d_mask", "mask_words", "d_depth", "window", "n_splits"]


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_argument_arrives_in_the_headers_position(entry):
    values = sentinels(entry)
    got = call(entry, values)
    check_plain(entry, values, got)
    for name, (ctype, _) in PER_SEQ.items():                              # sequences are copied into C arrays of the declared type
        assert isinstance(got[name], C.Array) and got[name]._type_ is ctype and list(got[name]) == values[name], name


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_none_and_zero_arrive_as_null(entry):
    values = sentinels(entry)
    nulled = [name for name in NULLABLE if name in values]
    values.update({name: None if name == "tail_idx" else 0 for name in nulled})
    got = call(entry, values)
    check_plain(entry, values, got, skip=nulled)
    assert got["tail_idx"] is None
    for name in nulled[1:]:
        assert isinstance(got[name], C.c_void_p) and got[name].value is None, name
    assert ("d_mask" in nulled) == ("d_mask" in [name for name, _ in declared(entry)])


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_numpy_arrays_arrive_by_their_own_data_pointer(entry):
    values = sentinels(entry)
    arrays = {name: np.asarray(values[name], dtype=dtype) for name, (_, dtype) in PER_SEQ.items()}
    values.update(arrays)
    got = call(entry, values)
    check_plain(entry, values, got)
    for name, a in arrays.items():                                        # no copy: the array's own memory
        assert isinstance(got[name], C.c_void_p) and got[name].value == a.ctypes.data, name
