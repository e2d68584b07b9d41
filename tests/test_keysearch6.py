"""IPv6 key search without a GPU: the C ABI's argument validation of the four entries (refused
before any device work) and the 320-row hill climb driven by the oracle."""
import ctypes

import numpy as np
import pytest

from rss_simulator_nvidia_amd import _native, keysearch

PTR = 0x1000  # never dereferenced: validation comes first


def words(seed, n):
    return np.random.RandomState(seed).randint(0, 2**32, (n, 9), dtype=np.uint32)


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("keys,nkeys,tuples,n,H,Q,counts,message", [
    (None, 2, PTR, 4, 128, 24, PTR, "or counts is NULL"),
    (PTR, 2, PTR, 4, 128, 24, None, "or counts is NULL"),
    (PTR, 0, PTR, 4, 128, 24, PTR, "no keys"),
    (PTR, 2, None, 4, 128, 24, PTR, "tuples is NULL"),
    (PTR, 2, PTR, 4, 0, 24, PTR, "must be >= 1"),
    (PTR, 2, PTR, 4, 128, 0, PTR, "must be >= 1"),
])
def test_search6_validation_before_any_device_work(entry, keys, nkeys, tuples, n, H, Q, counts,
                                                   message):
    lib = _native.load()
    if entry == "device":
        rc = lib.rss_key_search6_device(keys, nkeys, tuples, n, H, Q, counts, None)
    else:
        rc = lib.rss_key_search6_host(PTR, keys, nkeys, tuples, n, H, Q, counts)
    err = lib.rss_last_error().decode()
    assert rc == -22 and err.startswith("rss_key_search6_" + entry) and message in err, err


@pytest.mark.parametrize("key,tuples,n,H,Q,counts,message", [
    (None, PTR, 4, 128, 24, PTR, "key or counts is NULL"),
    ("example", PTR, 4, 128, 24, None, "key or counts is NULL"),
    ("example", None, 4, 128, 24, PTR, "tuples is NULL"),
    ("example", PTR, 4, 0, 24, PTR, "must be >= 1"),
    ("example", PTR, 4, 128, 0, PTR, "must be >= 1"),
    ("short", PTR, 4, 128, 24, PTR, "shorter than 40 bytes"),
    ("fields", PTR, 4, 128, 24, PTR, "field-selected"),
])
def test_neighbourhood6_validation_before_any_device_work(example_key, key, tuples, n, H, Q,
                                                          counts, message):
    lib = _native.load()
    keys = {"example": _native.prepare_key6(example_key),
            "short": _native.prepare_key6(list(example_key)[:39]),
            "fields": _native.prepare_key6(example_key, _native.FIELDS_IP)}
    k = ctypes.byref(keys[key]) if key else None
    for who, call in (
            ("device", lambda: lib.rss_key_neighbourhood6_device(k, tuples, n, H, Q, counts, None)),
            ("host", lambda: lib.rss_key_neighbourhood6_host(PTR, k, tuples, n, H, Q, counts))):
        assert call() == -22
        err = lib.rss_last_error().decode()
        assert err.startswith("rss_key_neighbourhood6_" + who) and message in err, err
    if key:  # the host entry also refuses a NULL context, once the rest is in order
        ok = ctypes.byref(keys["example"])
        assert lib.rss_key_neighbourhood6_host(None, ok, PTR, 4, 128, 24, PTR) == -22
        assert "context is NULL" in lib.rss_last_error().decode()


def test_neighbourhood6_accepts_a_40_byte_key(example_key):
    """The other side of the length check: 40 bytes pass, and n == 0 zeroes the counts on the
    host (no device is touched)."""
    lib = _native.load()
    key = _native.prepare_key6(list(example_key)[:40])
    counts = np.full((_native.KEY6_NEIGHBOURS, 24), 7, dtype=np.uint64)
    assert lib.rss_key_neighbourhood6_host(PTR, ctypes.byref(key), None, 0, 128, 24,
                                           counts.ctypes.data) == 0
    assert not counts.any()


def test_refine_ipv6_climbs_on_the_last_row(oracle_lib, example_key):
    H, Q = 100, 7
    tuples = words(5, 3000)

    def scorer(key):
        return np.stack([oracle_lib.run_words(keysearch.flip_bit(key, j), tuples, H, Q)[2]
                         for j in range(320)])

    start = keysearch.balance(oracle_lib.run_words(example_key, tuples, H, Q)[2], H, Q)
    r = keysearch.refine(example_key, tuples, H, Q, max_steps=3, neighbourhood=scorer, ipv6=True)
    np.testing.assert_array_equal(r["counts"], oracle_lib.run_words(r["key"], tuples, H, Q)[2])
    key = list(example_key)
    for j in r["flips"]:
        key = keysearch.flip_bit(key, j)
    assert r["flips"] and key == r["key"]
    assert (r["max_load"], r["chi2"]) < (start["max_load"][0], start["chi2"][0])
