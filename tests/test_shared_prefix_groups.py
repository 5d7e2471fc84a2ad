"""pplhip_op_shared_prefix_groups on hand-written page tables: a pure host function, no device needed."""
import numpy as np
import pytest

from tests.conftest import load_pplhip

X = 999  # an unused page-table entry


def groups(pages, start_pos, decoding, page_size, min_rows, min_tokens):
    m = load_pplhip()
    pages = np.ascontiguousarray(pages, dtype=np.int64)
    sp = np.ascontiguousarray(start_pos, dtype=np.int64)
    B = len(sp)
    group, tokens, n = np.full(B, 7, dtype=np.int32), np.zeros(max(B, 1), dtype=np.int64), np.zeros(1, dtype=np.int32)
    rc = m.lib().pplhip_op_shared_prefix_groups(pages.ctypes.data, pages.shape[1], sp.ctypes.data, B, decoding, page_size, min_rows, min_tokens,
                                                group.ctypes.data, tokens.ctypes.data, n.ctypes.data)
    assert rc == 0
    return group.tolist(), tokens[:n[0]].tolist()


CASES = {
    # rows 0, 2, 3 share pages 5, 6 (row 3 also 7 with row 0: not all rows); rows 1, 4 share page 9 only
    "two_buckets": (dict(pages=[[5, 6, 7, 1], [9, 20, 21, X], [5, 6, 30, X], [5, 6, 7, 2], [9, 22, X, X]],
                         start_pos=[50, 40, 40, 60, 20], decoding=5, page_size=16, min_rows=2, min_tokens=16),
                    ([0, 1, 0, 0, 1], [32, 16])),
    # row 2 is still inside page 1: the page of its current token is not shared
    "start_pos_clamps": (dict(pages=[[5, 6, 7, 1], [5, 6, 7, 2], [5, 6, X, X]], start_pos=[50, 60, 31], decoding=3, page_size=16, min_rows=2,
                              min_tokens=16), ([0, 0, 0], [16])),
    # ... and at start_pos 16 * k exactly, page k holds the current token
    "start_pos_on_page_edge": (dict(pages=[[5, 6, 7, 1], [5, 6, 7, 2]], start_pos=[32, 60], decoding=2, page_size=16, min_rows=2, min_tokens=16),
                               ([0, 0], [32])),
    "below_min_rows": (dict(pages=[[5, 6, 7], [5, 6, 8], [9, 1, 2]], start_pos=[40, 40, 40], decoding=3, page_size=16, min_rows=3, min_tokens=16),
                       ([-1, -1, -1], [])),
    "below_min_tokens": (dict(pages=[[5, 6, 7], [5, 6, 8]], start_pos=[40, 40], decoding=2, page_size=16, min_rows=2, min_tokens=33),
                         ([-1, -1], [])),
    # rows 2 and 3 are prefill rows: row 2 would join bucket 5 and, at start_pos 0, clamp it to nothing
    "prefill_ignored": (dict(pages=[[5, 6, 7], [5, 6, 8], [5, 6, 9], [5, 6, 3]], start_pos=[40, 40, 0, 40], decoding=2, page_size=16, min_rows=2,
                             min_tokens=16), ([0, 0, -1, -1], [32])),
    "page_size_32": (dict(pages=[[5, 6, 7], [5, 6, 8], [5, 6, 9]], start_pos=[70, 64, 95], decoding=3, page_size=32, min_rows=2, min_tokens=16),
                     ([0, 0, 0], [64])),
    "page_size_8_unsupported": (dict(pages=[[5, 6, 7], [5, 6, 8]], start_pos=[20, 20], decoding=2, page_size=8, min_rows=2, min_tokens=8),
                                ([-1, -1], [])),
    "off": (dict(pages=[[5, 6, 7], [5, 6, 8]], start_pos=[40, 40], decoding=2, page_size=16, min_rows=0, min_tokens=16), ([-1, -1], [])),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_prefix_groups(name):
    args, want = CASES[name]
    assert groups(**args) == want
