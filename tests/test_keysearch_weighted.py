"""Key search by load without a GPU: balance on weighted rows, the weighted entries' argument
validation (refused before any device work), the Python layer's weight checks, the CLI's
input flags, refine on loads driven by the oracle, and pcap packet counts."""
import ctypes

import numpy as np
import pytest

import pcap_builder as pb
from rss_simulator_nvidia_amd import _native, keysearch, pcap

PTR = 0x1000  # never dereferenced: validation comes first


def test_balance_ranks_loads_by_share():
    slots = np.array([6 if q < 8 else 5 for q in range(24)], dtype=np.uint64)
    perfect = slots * np.uint64(0xFFFFFFFF)  # any scale: rows are normalised by their sum
    heavy = perfect.copy()
    heavy[3] += perfect.sum()  # one elephant doubles the total on queue 3
    m = keysearch.balance(np.stack([perfect, heavy]), 128, 24)
    assert m["max_load"][0] == pytest.approx(1.0) and m["chi2"][0] == pytest.approx(0.0, abs=1e-3)
    assert m["max_load"][1] == pytest.approx((perfect[3] + perfect.sum()) / (2.0 * perfect[3]))
    assert list(m["used"]) == [24, 24]


@pytest.mark.parametrize("entry,change,message", [
    ("search", dict(loads=None), "or counts is NULL"), ("search", dict(keys=None), "or counts is NULL"),
    ("search", dict(nkeys=0), "no keys"), ("search", dict(tuples=None), "tuples is NULL"),
    ("search", dict(H=0), "must be >= 1"), ("search", dict(weights=None), "weights is NULL"),
    ("neighbourhood", dict(loads=None), "key or counts is NULL"),
    ("neighbourhood", dict(key="none"), "key or counts is NULL"),
    ("neighbourhood", dict(tuples=None), "tuples is NULL"),
    ("neighbourhood", dict(Q=0), "must be >= 1"),
    ("neighbourhood", dict(key="short"), "shorter than 16 bytes"),
    ("neighbourhood", dict(key="fields"), "field-selected"),
    ("neighbourhood", dict(weights=None), "weights is NULL")])
def test_validation_before_any_device_work(example_key, entry, change, message):
    lib = _native.load()
    a = dict(keys=PTR, nkeys=2, tuples=PTR, weights=PTR, n=4, H=128, Q=24, loads=PTR, key="example")
    a.update(change)
    keys = {"example": _native.prepare_key(example_key), "short": _native.prepare_key(range(15)),
            "fields": _native.prepare_key(example_key, "sd")}
    k = ctypes.byref(keys[a["key"]]) if a["key"] in keys else None
    tail = (a["n"], a["H"], a["Q"], a["loads"])
    calls = {
        "search_device": lambda: lib.rss_key_search_weighted_device(
            a["keys"], a["nkeys"], a["tuples"], a["weights"], *tail, None),
        "search_host": lambda: lib.rss_key_search_weighted_host(
            PTR, a["keys"], a["nkeys"], a["tuples"], a["weights"], *tail),
        "neighbourhood_device": lambda: lib.rss_key_neighbourhood_weighted_device(
            k, a["tuples"], a["weights"], *tail, None),
        "neighbourhood_host": lambda: lib.rss_key_neighbourhood_weighted_host(
            PTR, k, a["tuples"], a["weights"], *tail)}
    for who in ("device", "host"):
        assert calls[entry + "_" + who]() == -22
        err = lib.rss_last_error().decode()
        assert err.startswith("rss_key_%s_weighted_%s:" % (entry, who)) and message in err, err


@pytest.mark.parametrize("weights,message", [
    ([1, 2, 3], "one weight per tuple"), ([1, 2, 3, -1], r"\[0, 2\^32\)"),
    ([1, 2, 3, 2**32], r"\[0, 2\^32\)"), ([1.0, 2.0, 3.0, 4.5], "integers")])
def test_python_layer_refuses_bad_weights(weights, message):
    with pytest.raises(ValueError, match=message):
        _native.tuple_weights(np.array(weights), 4)
    ok = _native.tuple_weights(np.array([0, 1, 2**32 - 1, 7]), 4)
    assert ok.dtype == np.uint32 and list(ok) == [0, 1, 2**32 - 1, 7]


@pytest.mark.parametrize("call", ["evaluate", "search", "neighbourhood", "refine"])
def test_ipv6_with_weights_is_not_implemented(call):
    t6, w = np.zeros((2, 9), dtype=np.uint32), np.ones(2, dtype=np.uint32)
    key = list(range(40))
    with pytest.raises(NotImplementedError, match="IPv4 tuples only"):
        {"evaluate": lambda: keysearch.evaluate([key], t6, 128, 24, ipv6=True, weights=w),
         "search": lambda: keysearch.search(t6, 128, 24, n_keys=2, ipv6=True, weights=w),
         "neighbourhood": lambda: keysearch.neighbourhood(key, t6, 128, 24, ipv6=True, weights=w),
         "refine": lambda: keysearch.refine(key, t6, 128, 24, ipv6=True, weights=w)}[call]()


@pytest.mark.parametrize("argv,message", [
    ([], "one of the arguments --ips-file --pcap is required"),
    (["--ips-file", "a.csv", "--pcap", "b.pcap"], "not allowed with argument"),
    (["--pcap", "b.pcap", "--weight-column", "packets"], "not allowed with --pcap"),
    (["--pcap", "b.pcap", "--ipv6"], "IPv4 flows only"),
    (["--ips-file", "CSV", "--weight-column", "nope"], "has no column 'nope'"),
    (["--ips-file", "CSV", "--weight-column", "bad"], r"\[0, 2\^32\)")])
def test_cli_input_flags(argv, message, tmp_path, capsys):
    csv = tmp_path / "flows.csv"
    csv.write_text("src_ip,dst_ip,src_port,dst_port,packets,bad\n1.1.1.1,2.2.2.2,1,2,9,-1\n")
    argv = [str(csv) if a == "CSV" else a for a in argv]
    with pytest.raises(SystemExit) as stop:
        keysearch.main(argv + ["--htable-size", "128", "--num-queues", "24"])
    err = capsys.readouterr().err
    assert stop.value.code == 2 and err.startswith("usage: rss-keysearch")
    assert __import__("re").search(message, err), err


def test_refine_on_loads_with_a_numpy_neighbourhood(oracle_lib, example_key):
    H, Q = 100, 7
    tuples = oracle_lib.generate(5, 0, 5000)
    weights = np.minimum(np.random.default_rng(2).zipf(1.3, len(tuples)), 2**32 - 1).astype(np.uint64)

    def loads(key):
        return np.bincount(oracle_lib.run(key, tuples, H, Q)[1], weights=weights.astype(np.float64),
                           minlength=Q).astype(np.uint64)  # sums stay far below 2^53

    def scorer(key):
        return np.stack([loads(keysearch.flip_bit(key, j)) for j in range(128)])

    start = keysearch.balance(loads(example_key), H, Q)
    r = keysearch.refine(example_key, tuples, H, Q, neighbourhood=scorer, weights=weights)
    np.testing.assert_array_equal(r["counts"], loads(r["key"]))
    assert r["flips"] and r["counts"].sum() == weights.sum()
    assert (r["max_load"], r["chi2"]) < (start["max_load"][0], start["chi2"][0])


def test_pcap_packet_counts_follow_first_seen_order(tmp_path):
    flows = [((10, 0, 0, 1), (10, 0, 0, 9), 5000, 80), ((10, 0, 0, 2), (10, 0, 0, 9), 5001, 443),
             ((9, 9, 9, 9), (1, 1, 1, 1), 7, 7)]
    order = [1, 0, 1, 2, 1, 0, 1]  # flow 1 first (4 packets), then 0 (2), then 2 (1)
    packets = [pb.ether(pb.ipv4(flows[f][0], flows[f][1], 17, pb.l4(flows[f][2], flows[f][3])))
               for f in order]
    path = tmp_path / "flows.pcap"
    path.write_bytes(pb.pcap_file(packets))
    plain = pcap.read_flows(str(path))
    tuples, protos, skipped, counts = pcap.read_flows(str(path), packet_counts=True)
    assert len(plain) == 3 and np.array_equal(plain[0], tuples) and skipped == 0
    assert counts.dtype == np.uint32 and list(counts) == [4, 2, 1] and counts.sum() == len(packets)
    assert [int(p) & 0xFFFF for p in tuples["ports"]] == [443, 80, 7]
    every = pcap.read_flows(str(path), unique=False, packet_counts=True)
    assert len(every[0]) == len(packets) and list(every[3]) == [1] * len(packets)
