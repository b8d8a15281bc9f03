"""Per-image Huffman tables, host part (no GPU): tic_huffman_table_build against the reference's calc_huffman_table and
write_huffman_table (huffman.py:101-194, codec.py:73-84) on crafted histograms - equal counts, Fibonacci counts, one and two symbols,
many counts of 1, ties (tests/golden/adaptive_streams.json, made by tests/golden/gen/make_goldens_adaptive.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tinyimgcodec_amd import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture():
    with open(os.path.join(GOLDEN, "adaptive_streams.json")) as f:
        return json.load(f)


def build(dc, ac, table_cap=4096):
    """dc / ac: lists of [bin, count, first key] -> (rc, dc codes, ac codes, table bytes, table bits)."""
    L = N.load()
    cnt = {k: np.zeros(n, np.uint64) for k, n in (("dc", 16), ("ac", 256))}
    first = {k: np.full(n, np.iinfo(np.uint64).max, np.uint64) for k, n in (("dc", 16), ("ac", 256))}
    for k, rows in (("dc", dc), ("ac", ac)):
        for b, c, f in rows:
            cnt[k][b] = c
            first[k][b] = f
    dc_code, ac_code = np.zeros(16, np.uint64), np.zeros(256, np.uint64)
    dc_len, ac_len = np.zeros(16, np.uint8), np.zeros(256, np.uint8)
    table = np.zeros(max(table_cap, 1), np.uint8)
    nbits = C.c_size_t(0)
    rc = L.tic_huffman_table_build(cnt["dc"].ctypes.data, first["dc"].ctypes.data, cnt["ac"].ctypes.data, first["ac"].ctypes.data,
                                   dc_code.ctypes.data, dc_len.ctypes.data, ac_code.ctypes.data, ac_len.ctypes.data, table.ctypes.data,
                                   table_cap, C.byref(nbits))
    return rc, (dc_code, dc_len), (ac_code, ac_len), table, nbits.value


def as_string(code, n):
    return format(int(code), "0%db" % n) if n else ""


@pytest.mark.parametrize("case", _fixture()["tables"], ids=lambda c: c["name"])
def test_table_build_matches_reference(case):
    rc, (dcc, dcl), (acc, acl), table, nbits = build(case["dc"], case["ac"])
    assert rc == N.TIC_OK
    for b, code in case["dc_codes"]:
        assert as_string(dcc[b], dcl[b]) == code, ("DC", b)
    for b, code in case["ac_codes"]:
        assert as_string(acc[b], acl[b]) == code, ("AC", b)
    assert {b for b, _, _ in case["dc"]} == {b for b, _ in case["dc_codes"]}
    assert {b for b, _, _ in case["ac"]} == {b for b, _ in case["ac_codes"]}
    # symbols that do not occur get no code
    assert all(dcl[b] == 0 for b in range(16) if b not in {r[0] for r in case["dc"]})
    assert all(acl[b] == 0 for b in range(256) if b not in {r[0] for r in case["ac"]})
    # serialized table (entries in the tree's depth-first leaf order), zero-padded to a byte
    assert nbits == case["table_bits"]
    assert table[: (nbits + 7) // 8].tobytes().hex() == case["table"]


def test_table_build_first_occurrence_decides_ties():
    """Equal counts: only the first-occurrence keys differ, and the codes follow them (heapq order of the leaves)."""
    ac = [[0x01, 3, 0], [0x02, 3, 1], [0x00, 3, 2]]
    swapped = [[0x01, 3, 2], [0x02, 3, 1], [0x00, 3, 0]]
    dc = [[0, 1, 0]]
    a = build(dc, ac)
    b = build(dc, swapped)
    assert a[0] == b[0] == N.TIC_OK
    assert [as_string(a[2][0][s], a[2][1][s]) for s in (1, 2, 0)] != [as_string(b[2][0][s], b[2][1][s]) for s in (1, 2, 0)]


def test_table_build_errors():
    rc = build([], [[0, 1, 0]])[0]
    assert rc == N.TIC_E_ARG  # no DC symbol (the reference: IndexError)
    rc = build([[0, 1, 0]], [])[0]
    assert rc == N.TIC_E_ARG
    case = _fixture()["tables"][0]
    rc = build(case["dc"], case["ac"], table_cap=(case["table_bits"] + 7) // 8 - 1)[0]
    assert rc == N.TIC_E_SPACE
    # Fibonacci counts over 60 AC symbols: a tree 59 deep, past what code plus value bits may take (64)
    fib = [1, 1]
    while len(fib) < 60:
        fib.append(fib[-1] + fib[-2])
    ac = [[(r << 4) | s, fib[k], k] for k, (r, s) in enumerate([(r, s) for r in range(6) for s in range(10, 0, -1)])]
    rc = build([[0, 1, 0]], ac)[0]
    assert rc == N.TIC_E_RANGE
