"""The host plumbing every C-ABI wrapper shares (emotiongestures_amd._host), without a GPU: host integer vectors, the bounded build-once
cache and numpy host pointers."""
import numpy as np
import pytest
import torch

from emotiongestures_amd import _host as H

VALUES = [3, 0, 7, 2 ** 31 - 1, -1]


@pytest.mark.parametrize("make", [list, tuple, lambda v: np.asarray(v, np.int32), lambda v: np.asarray(v, np.int64),
                                  lambda v: torch.tensor(v, dtype=torch.int64)], ids=["list", "tuple", "int32", "int64", "tensor"])
def test_int_list_same_python_ints(make):
    out = H.int_list(make(VALUES))
    assert out == VALUES and all(type(a) is int for a in out)


def test_int_list_range_empty_and_bare_int():
    out = H.int_list(range(4))
    assert out == [0, 1, 2, 3] and all(type(a) is int for a in out)
    for empty in ([], (), range(0), np.zeros(0, np.int32), torch.zeros(0, dtype=torch.int64)):
        assert H.int_list(empty) == []
    with pytest.raises(TypeError):
        H.int_list(5)


def test_bounded_cache_drops_the_oldest_insertion():
    built = []

    def get(cache, key):
        return cache.get(key, lambda: built.append(key) or key.upper())

    c = H.BoundedCache(limit=3)
    for key in "abcd":
        assert get(c, key) == key.upper()
    assert "a" not in c and all(k in c for k in "bcd") and len(c) == 3
    for key in "bcdbcd":                                    # hits: nothing is built again, and a hit does not refresh an entry (FIFO, not LRU)
        get(c, key)
    assert built == list("abcd")
    assert get(c, "a") == "A" and built == list("abcda")    # a was dropped: built again, and b, the oldest insertion, goes
    assert "b" not in c and all(k in c for k in "cda") and len(c) == 3


def test_bounded_cache_without_limit_keeps_everything():
    c = H.BoundedCache(limit=None)
    for k in range(100):
        c.get(k, lambda: k)
    assert len(c) == 100 and all(k in c for k in range(100))


def test_host_ptr():
    a = np.arange(6, dtype=np.int32)
    assert H.host_ptr(None) is None
    assert H.host_ptr(a).value == a.ctypes.data


def test_sized_returns_the_bytes_or_raises_with_the_last_error():
    from emotiongestures_amd import _lib as L
    assert H.sized("eg_srgr_workspace_bytes", 2, 20, 5) == (8 + 4 * 5) * 2
    with pytest.raises(L.EgError) as e:
        H.sized("eg_srgr_workspace_bytes", 2, 20, 65)
    assert str(e.value) == "eg_srgr_workspace_bytes: refused (eg_srgr_workspace_bytes: joints=65 (1..64))"
    with pytest.raises(L.EgError, match=r"^eg_kin_workspace_bytes: refused \(eg_kin_workspace_bytes: frames=3 \(need >= 4"):
        H.sized("eg_kin_workspace_bytes", 2, 3, 5, 40)


def test_count_list_keeps_the_callers_words():
    from emotiongestures_amd import _rows as RW
    assert RW.count_list(np.asarray([4, 5], np.int64), 2, "pack_rows") == [4, 5]
    with pytest.raises(ValueError) as e:
        RW.count_list([4, 5, 6], 2, "pack_rows")
    assert str(e.value) == "pack_rows: frames has 3 entries for 2 recordings"
    with pytest.raises(ValueError) as e:
        RW.count_list(torch.tensor([7]), 2, "beat_alignment_tracks", "t_end")
    assert str(e.value) == "beat_alignment_tracks: t_end has 1 entries for 2 recordings"
    assert RW.counts32(None) is None
    c = RW.counts32([3, 4])
    assert c.dtype == np.int32 and c.flags["C_CONTIGUOUS"] and c.tolist() == [3, 4]
