"""Host-side surface of the homogeneous room stream and the per-graph counts: the new entries are exported and bound, the ABI version
is unchanged, and ``hmp_collator_set_label_filter`` (host code, like the collator's create / destroy) validates its arguments
without a device."""
import ctypes as C
import os
import re

import numpy as np

from hydra_gnn_amd import _lib

NEW = ("hmp_collator_set_label_filter", "hmp_count_correct_rows_by_graph", "hmp_net_count_correct_rooms_by_graph")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hydra_mp.h")


def test_new_entries_are_declared_exported_and_bound():
    lib = _lib.load()
    with open(HEADER) as f:
        text = f.read()
    for name in NEW:
        assert re.search(r"^int\s+" + name + r"\(", text, re.M), name
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(_lib.SIGNATURES[name][1])
    assert lib.hmp_abi_version() == 4
    assert C.sizeof(_lib.CollateItem) == 48  # the label filter is a collator setting: the public item keeps its layout


def _collator(lib):
    """a collator over fake device addresses (never dereferenced on the host): item 0 = 24-byte rows, 1 = int64 labels, 2 = byte
    rows, 3 = an edge list"""
    ptr = np.array([0, 3, 5], dtype=np.int64)
    slot_ptr = (C.c_void_p * 2)(ptr.ctypes.data, ptr.ctypes.data)
    items = (_lib.CollateItem * 4)(_lib.CollateItem(0x1000, 0x2000, 0, 24, 0, 0, 0), _lib.CollateItem(0x3000, 0x2000, 0, 8, 0, 0, 0),
                                   _lib.CollateItem(0x4000, 0x2000, 0, 1, 0, 0, 0), _lib.CollateItem(0x5000, 0x6000, 5, 0, 1, 0, 0))
    h = C.c_void_p()
    _lib.check(lib.hmp_collator_create(2, slot_ptr, 2, 4, items, C.byref(h)))
    return h, (ptr, slot_ptr, items)


def test_label_filter_validates_its_item_without_a_device():
    lib = _lib.load()
    h, keep = _collator(lib)
    try:
        assert lib.hmp_collator_set_label_filter(h, 1, 0x7000, 25) == 0
        assert lib.hmp_collator_set_label_filter(h, -1, None, 0) == 0  # clears
        for item, mask, word in ((0, 0x7000, b"bytes"), (2, 0x7000, b"bytes"), (3, 0x7000, b"bytes"), (4, 0x7000, b"item"),
                                 (1, None, b"mask")):
            rc = lib.hmp_collator_set_label_filter(h, item, mask, 25)
            assert rc == 1, (item, rc)  # HMP_E_ARG
            msg = lib.hmp_last_error()
            assert b"hmp_collator_set_label_filter" in msg and word in msg, msg
        assert lib.hmp_collator_set_label_filter(None, 1, 0x7000, 25) == 1
    finally:
        lib.hmp_collator_destroy(h)
