"""Symmetric RSS without a GPU: the key bytes, every entry's argument validation (refused
before any device work) and the CLI's flags."""
import ctypes
import re

import pytest

from rss_simulator_nvidia_amd import _native, keysearch

PTR = 0x1000  # never dereferenced: validation comes first


def test_symmetric_key_bytes():
    assert keysearch.symmetric_key(0x6d5a) == [0x6d, 0x5a] * 20
    assert keysearch.symmetric_key(0x0180, 52) == [0x01, 0x80] * 26
    assert keysearch.key_text(keysearch.symmetric_key(0xFFFF, 4)) == "ff:ff:ff:ff"
    lib, buf = _native.load(), (ctypes.c_uint8 * 64)()
    for length in (0, 2, 41, 54):  # odd or outside [4, 52]
        assert lib.rss_symmetric_key(1, buf, length) == -22
        assert "rss_symmetric_key: len must be even" in lib.rss_last_error().decode()


@pytest.mark.parametrize("entries,change,message", [
    (("fold_device",), dict(folds=None), "folds is NULL"),
    (("search_device",), dict(folds=None), "folds or loads is NULL"),
    (("search_device", "search_host"), dict(loads=None), "loads is NULL"),
    (("search_host",), dict(ctx=None), "context is NULL"),
    (("fold_device", "search_host"), dict(tuples=None), "tuples is NULL"),
    (("fold_device", "search_host"), dict(words=4), "words must be 3 (IPv4) or 9 (IPv6), got 4"),
    (("fold_device", "search_host"), dict(fields=0), "bad field mask 0x0"),
    (("fold_device", "search_host"), dict(fields=16), "bad field mask 0x10"),
    (("search_device", "search_host"), dict(count=0), "no patterns"),
    (("search_device", "search_host"), dict(first=65530, count=7), "patterns [65530, 65537) exceed"),
    (("search_device", "search_host"), dict(H=0), "must be >= 1"),
    (("search_device", "search_host"), dict(Q=0), "must be >= 1")])
def test_validation_before_any_device_work(entries, change, message):
    lib = _native.load()
    a = dict(ctx=PTR, tuples=PTR, words=3, fields=15, weights=None, n=4, folds=PTR, first=0,
             count=16, H=128, Q=24, loads=PTR)
    a.update(change)
    calls = {
        "fold_device": lambda: lib.rss_symmetric_fold_device(
            a["tuples"], a["words"], a["fields"], a["weights"], a["n"], a["folds"], 0, None),
        "search_device": lambda: lib.rss_symmetric_search_device(
            a["folds"], a["first"], a["count"], a["H"], a["Q"], a["loads"], None),
        "search_host": lambda: lib.rss_symmetric_search_host(
            a["ctx"], a["tuples"], a["words"], a["fields"], a["weights"], a["n"], a["first"],
            a["count"], a["H"], a["Q"], a["loads"])}
    for who in entries:
        assert calls[who]() == -22
        err = lib.rss_last_error().decode()
        assert err.startswith("rss_symmetric_%s:" % who) and message in err, err


@pytest.mark.parametrize("argv,message", [
    (["--ips-file", "a.csv", "--symmetric", "--refine", "4"], "breaks the key's symmetry"),
    (["--pcap", "b.pcap", "--ipv6"], "IPv4 flows only"),
    (["--ips-file", "a.csv", "--ipv6", "--weight-column", "packets"], "IPv4 flows only")])
def test_cli_flags(argv, message, capsys):
    with pytest.raises(SystemExit) as stop:
        keysearch.main(argv + ["--htable-size", "128", "--num-queues", "24"])
    err = capsys.readouterr().err
    assert stop.value.code == 2 and re.search(message, err), err
