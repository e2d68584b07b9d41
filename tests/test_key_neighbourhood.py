"""Key neighbourhood and refine without a GPU: the C ABI's argument validation (refused
before any device work), flip_bit, and the hill climb driven by the oracle."""
import ctypes

import numpy as np
import pytest

from rss_simulator_nvidia_amd import _native, keysearch

PTR = 0x1000  # never dereferenced: validation comes first


@pytest.mark.parametrize("key,tuples,n,H,Q,counts,message", [
    (None, PTR, 4, 128, 24, PTR, "key or counts is NULL"),
    ("example", PTR, 4, 128, 24, None, "key or counts is NULL"),
    ("example", None, 4, 128, 24, PTR, "tuples is NULL"),
    ("example", PTR, 4, 0, 24, PTR, "must be >= 1"),
    ("example", PTR, 4, 128, 0, PTR, "must be >= 1"),
    ("short", PTR, 4, 128, 24, PTR, "shorter than 16 bytes"),
    ("fields", PTR, 4, 128, 24, PTR, "field-selected"),
])
def test_validation_before_any_device_work(example_key, key, tuples, n, H, Q, counts, message):
    lib = _native.load()
    keys = {"example": _native.prepare_key(example_key), "short": _native.prepare_key(range(15)),
            "fields": _native.prepare_key(example_key, "sd")}
    k = ctypes.byref(keys[key]) if key else None
    for who, call in (("device", lambda: lib.rss_key_neighbourhood_device(k, tuples, n, H, Q, counts, None)),
                      ("host", lambda: lib.rss_key_neighbourhood_host(PTR, k, tuples, n, H, Q, counts))):
        assert call() == -22
        err = lib.rss_last_error().decode()
        assert err.startswith("rss_key_neighbourhood_" + who) and message in err, err


def test_flip_bit():
    key = list(range(40))
    assert keysearch.flip_bit(key, 0)[0] == 0x80 and keysearch.flip_bit(key, 7)[0] == 0x01
    assert keysearch.flip_bit(key, 127)[15] == 15 ^ 0x01
    assert keysearch.flip_bit(keysearch.flip_bit(key, 77), 77) == key == list(range(40))
    assert sum(a != b for a, b in zip(keysearch.flip_bit(key, 77), key)) == 1


def test_refine_reaches_a_local_optimum(oracle_lib, example_key):
    H, Q = 100, 7
    tuples = oracle_lib.generate(5, 0, 5000)

    def scorer(key):
        return np.stack([oracle_lib.run(keysearch.flip_bit(key, j), tuples, H, Q)[2]
                         for j in range(128)])

    start = keysearch.balance(oracle_lib.run(example_key, tuples, H, Q)[2], H, Q)
    r = keysearch.refine(example_key, tuples, H, Q, neighbourhood=scorer)
    np.testing.assert_array_equal(r["counts"], oracle_lib.run(r["key"], tuples, H, Q)[2])
    key = list(example_key)
    for j in r["flips"]:
        key = keysearch.flip_bit(key, j)
    assert r["flips"] and key == r["key"]
    assert (r["max_load"], r["chi2"]) < (start["max_load"][0], start["chi2"][0])
    m = keysearch.balance(scorer(r["key"]), H, Q)  # no row beats the result
    assert min(zip(m["max_load"], m["chi2"])) >= (r["max_load"], r["chi2"])
    capped = keysearch.refine(example_key, tuples, H, Q, max_steps=1, neighbourhood=scorer)
    assert capped["flips"] == r["flips"][:1]
