"""Go 1.16 sort.Slice on its own: gosort.h as the Preemptor's kernels run it
(go_sort_keyed, key[x] < key[y] over an index list; pe_probe_go_sort) against
the oracle's GoSort, on the host and on the device, with both index types the
kernels instantiate (uint8_t up to 255 elements, uint16_t).

The sort is not stable and the preempted set depends on its order of equal
keys, so the permutations are compared exactly. Random keys never reach
heapSort_func (the depth limit is 2 * ceil(log2(n + 1)) pivots): the inputs that
do are McIlroy's adversary ("A Killer Adversary for Quicksort", 1999) run
against the oracle's GoSort, replayed as plain keys, and the same ranks halved
so that the heap-sorted range holds equal keys. The oracle counts its
heapSort_func calls; the tests assert the counts, so a changed generator cannot
empty them silently.
"""
import ctypes as C
import os

import numpy as np
import pytest

from nomad_amd import abi
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nomad_amd", "libnomadpe.so")

SIZES = [0, 1, 2, 6, 7, 12, 13, 40, 41, 42, 64, 100, 128, 250, 255, 256, 1024, 2048]
PATTERNS = ["distinct", "three", "equal", "ascending", "descending", "organ_pipe", "killer", "killer_halved", "nan"]
# heapSort_func is reached by the distinct killer at every listed n >= 40 and by
# the halved one at these n (the oracle's counter decides; asserted below)
KILLER_REACHES = [n for n in SIZES if n >= 40]
HALVED_REACHES = [40, 100, 128, 250, 255, 256, 1024, 2048]


def make_keys(pattern, n):
    rng = np.random.Generator(np.random.PCG64(1000 * PATTERNS.index(pattern) + n))
    if pattern == "distinct":
        return rng.permutation(n).astype(np.float64)
    if pattern == "three":
        return rng.integers(0, 3, size=n).astype(np.float64)
    if pattern == "equal":
        return np.full(n, 0.25)
    if pattern == "ascending":
        return np.arange(n, dtype=np.float64)
    if pattern == "descending":
        return np.arange(n, dtype=np.float64)[::-1].copy()
    if pattern == "organ_pipe":
        return np.minimum(np.arange(n), n - 1 - np.arange(n)).astype(np.float64)
    if pattern == "killer":
        return oracle.sort_killer(n).copy()
    if pattern == "killer_halved":
        return np.floor(oracle.sort_killer(n) / 2.0)
    if pattern == "nan":   # the comparator is unordered both ways at a NaN key (evict.inc)
        k = rng.integers(0, max(1, n // 2), size=n).astype(np.float64)
        if n:
            k[rng.integers(0, n, size=max(1, n // 16))] = np.nan
        return k
    raise ValueError(pattern)


CASES = [(p, n) for n in SIZES for p in PATTERNS]
KEYS = {c: make_keys(*c) for c in CASES}
_cache = {}


def oracle_perms():
    if "oracle" not in _cache:
        _cache["oracle"] = {c: oracle.go_sort(KEYS[c]).copy() for c in CASES}
    return _cache["oracle"]


def probe_sort(cases, width, device):
    """pe_probe_go_sort over the cases' key arrays in one call; {case: permutation}."""
    lib = abi.bind_probes(C.CDLL(LIB))
    off = np.concatenate([[0], np.cumsum([len(KEYS[c]) for c in cases])]).astype(np.uint32)
    keys = np.ascontiguousarray(np.concatenate([KEYS[c] for c in cases]))
    perm = np.full(max(1, len(keys)), 0xFFFFFFFF, dtype=np.uint32)
    rc = lib.pe_probe_go_sort(keys.ctypes.data_as(abi.f64p), off.ctypes.data_as(abi.u32p), len(cases), width,
                              perm.ctypes.data_as(abi.u32p), device)
    assert rc == 0, rc
    return {c: perm[off[i]:off[i + 1]].copy() for i, c in enumerate(cases)}


def cases_of(width):
    return [c for c in CASES if width == 2 or c[1] <= 255]


def host_perms(width):
    if width not in _cache:
        _cache[width] = probe_sort(cases_of(width), width, 0)
    return _cache[width]


# ---- CPU ----------------------------------------------------------------------------

@pytest.mark.parametrize("width", [1, 2])
def test_host_sort_equals_oracle(width):
    want = oracle_perms()
    got = host_perms(width)
    assert len(got) == (len(CASES) if width == 2 else len(PATTERNS) * sum(n <= 255 for n in SIZES))
    for c in cases_of(width):
        assert np.array_equal(got[c], want[c]), c


@pytest.mark.parametrize("which", ["oracle", 1, 2])
def test_output_is_a_sorted_permutation(which):
    """Independent of either implementation: a permutation of 0..n-1 that leaves
    NaN-free keys non-decreasing."""
    perms = oracle_perms() if which == "oracle" else host_perms(which)
    for c, p in perms.items():
        assert np.array_equal(np.sort(p), np.arange(c[1])), c
        if c[0] != "nan":
            assert (np.diff(KEYS[c][p]) >= 0).all(), c


def heap_stats_of(keys):
    oracle.sort_heap_reset()
    oracle.go_sort(keys)
    return oracle.sort_heap_stats()


def test_killer_inputs_reach_heapsort():
    assert len(KILLER_REACHES) >= 3 and len(HALVED_REACHES) >= 2
    for n in SIZES:
        calls, elems, ties = heap_stats_of(KEYS[("killer", n)])
        assert (calls > 0) == (n in KILLER_REACHES), (n, calls)
        assert ties == 0 and (calls == 0 or 12 < elems <= n), (n, calls, elems, ties)
        calls, elems, ties = heap_stats_of(KEYS[("killer_halved", n)])
        assert (calls > 0) == (n in HALVED_REACHES), (n, calls)
        assert (ties > 0) == (n in HALVED_REACHES), (n, ties)   # equal keys inside the heap-sorted range
    # the ranges the issue's replay measured
    assert heap_stats_of(KEYS[("killer", 41)])[:2] == (1, 14)
    assert heap_stats_of(KEYS[("killer", 250)])[:2] == (1, 170)
    assert heap_stats_of(KEYS[("killer", 1024)])[:2] == (1, 914)
    for n in (128, 250, 1024):
        assert n in HALVED_REACHES


def test_other_patterns_never_reach_heapsort():
    oracle.sort_heap_reset()
    for c in CASES:
        if not c[0].startswith("killer") and c[0] != "nan":
            oracle.go_sort(KEYS[c])
    assert oracle.sort_heap_stats() == (0, 0, 0)


def test_probe_rejects_bad_arguments():
    lib = abi.bind_probes(C.CDLL(LIB))
    keys = np.zeros(300)
    perm = np.zeros(300, dtype=np.uint32)

    def call(off, width):
        o = np.array(off, dtype=np.uint32)
        return lib.pe_probe_go_sort(keys.ctypes.data_as(abi.f64p), o.ctypes.data_as(abi.u32p), len(off) - 1, width,
                                    perm.ctypes.data_as(abi.u32p), 0)
    assert call([0, 255], 1) == 0
    assert call([0, 256], 1) == -1      # past the byte index type
    assert call([0, 300], 2) == 0
    assert call([0, 10], 3) == -1
    assert call([1, 10], 2) == -1
    assert call([0, 10, 5], 2) == -1


# ---- GPU ----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 2])
def test_device_sort_equals_host(width):
    """One lane per array, every pattern and size in one launch."""
    want = host_perms(width)
    got = probe_sort(cases_of(width), width, 1)
    for c in cases_of(width):
        assert np.array_equal(got[c], want[c]), c
