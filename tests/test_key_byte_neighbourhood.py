"""The byte neighbourhood without a GPU: the six entries' argument validation (refused before
any device work) and refine(step="byte") driven by the oracle."""
import ctypes

import numpy as np
import pytest

from rss_simulator_nvidia_amd import _native, keysearch

PTR = 0x1000  # never dereferenced: validation comes first

CAUSES = [
    (dict(out=None), "key or counts is NULL"), (dict(key="none"), "key or counts is NULL"),
    (dict(tuples=None), "tuples is NULL"), (dict(H=0), "must be >= 1"), (dict(Q=0), "must be >= 1"),
    (dict(key="short"), "shorter than"), (dict(key="fields"), "field-selected"),
    (dict(nbytes=0), "nbytes is 0"), (dict(first=1, nbytes="all"), "exceed the"),
    (dict(ctx=None), "context is NULL")]


@pytest.mark.parametrize("entry,change,message", [(e, c, m) for e in ("", "6", "_weighted")
                                                  for c, m in CAUSES] +
                         [("_weighted", dict(weights=None), "weights is NULL")])
def test_validation_before_any_device_work(example_key, entry, change, message):
    lib = _native.load()
    six = entry == "6"
    total = _native.KEY6_BYTES if six else _native.KEY_BYTES
    a = dict(key="example", first=0, nbytes=total, tuples=PTR, weights=PTR, H=128, Q=24, out=PTR,
             ctx=PTR)
    a.update(change)
    if a["nbytes"] == "all":  # first_byte + nbytes = 17 (IPv6: 41)
        a["nbytes"] = total
    prepare = _native.prepare_key6 if six else _native.prepare_key
    keys = {"example": prepare(example_key), "short": prepare(list(range(total - 1))),
            "fields": prepare(example_key, "sd")}
    k = ctypes.byref(keys[a["key"]]) if a["key"] in keys else None
    args = (k, a["first"], a["nbytes"], a["tuples"]) + ((a["weights"],) if entry == "_weighted"
                                                        else ()) + (4, a["H"], a["Q"], a["out"])
    calls = [("host", lambda f: f(a["ctx"], *args))]
    if "ctx" not in change:  # the device entries take no context
        calls.append(("device", lambda f: f(*args, None)))
    for who, call in calls:
        name = "rss_key_byte_neighbourhood%s_%s" % (entry, who)
        assert call(getattr(lib, name)) == -22
        err = lib.rss_last_error().decode()
        assert err.startswith(name + ":") and message in err, err


def test_refine_by_bytes_with_a_numpy_neighbourhood(oracle_lib, example_key):
    H, Q = 100, 7
    tuples = oracle_lib.generate(5, 0, 5000)

    def counts(key):
        return oracle_lib.run(key, tuples, H, Q, want_hash=False, want_queue=False)[2]

    def byte_rows(key):
        return np.stack([counts(key[:B] + [v] + key[B + 1:]) for B in range(16) for v in range(256)])

    def bit_rows(key):
        return np.stack([counts(keysearch.flip_bit(key, j)) for j in range(128)])

    start = keysearch.balance(counts(example_key), H, Q)
    r = keysearch.refine(example_key, tuples, H, Q, max_steps=1, neighbourhood=byte_rows,
                         step="byte")
    np.testing.assert_array_equal(r["counts"], counts(r["key"]))
    (B, v), = r["moves"]
    assert r["flips"] == [] and r["key"] == example_key[:B] + [v] + example_key[B + 1:]
    assert (r["max_load"], r["chi2"]) < (start["max_load"][0], start["chi2"][0])
    # the bit rows are a subset of the byte rows: one byte step dominates one bit step
    bit = keysearch.refine(example_key, tuples, H, Q, max_steps=1, neighbourhood=bit_rows)
    assert (r["max_load"], r["chi2"]) <= (bit["max_load"], bit["chi2"])
    with pytest.raises(NotImplementedError, match="IPv4 tuples only"):
        keysearch.byte_neighbourhood(list(range(40)), np.zeros((2, 9), np.uint32), 128, 24,
                                     ipv6=True, weights=np.ones(2, np.uint32))
