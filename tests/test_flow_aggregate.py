"""Flow aggregation without a GPU: every entry's argument validation (refused before any device
work), the workspace size and the CLI's flags."""
import ctypes
import re

import pytest

from rss_simulator_nvidia_amd import _native, keysearch

PTR = 0x1000  # never dereferenced: validation comes first
BIG = (1 << 30) + 1


@pytest.mark.parametrize("entries,change,message", [
    (("workspace_bytes", "device", "host"), dict(words=4), "words must be 3 (IPv4) or 9 (IPv6), got 4"),
    (("workspace_bytes", "device", "host"), dict(n=BIG), "1073741825 packets exceed the limit of 2^30"),
    (("workspace_bytes",), dict(out=None), "NULL argument"),
    (("device", "host"), dict(tuples=None), "tuples is NULL"),
    (("device", "host"), dict(nflows=None), "nflows is NULL"),
    (("device", "host"), dict(flows=None), "flows, loads or first is NULL"),
    (("device", "host"), dict(loads=None), "flows, loads or first is NULL"),
    (("device", "host"), dict(first=None), "flows, loads or first is NULL"),
    (("device",), dict(ws=None), "workspace NULL or not 8-byte aligned"),
    (("device",), dict(ws=PTR + 4), "workspace NULL or not 8-byte aligned"),
    (("device",), dict(ws_bytes=12311), "workspace of 12311 bytes, 4 packets need 12312"),
    (("host",), dict(ctx=None), "context is NULL")])
def test_validation_before_any_device_work(entries, change, message):
    lib, size = _native.load(), ctypes.c_size_t()
    a = dict(ctx=PTR, tuples=PTR, words=3, weights=None, n=4, flows=PTR, loads=PTR, first=PTR,
             nflows=PTR, ws=PTR, ws_bytes=1 << 20, out=ctypes.byref(size))
    a.update(change)
    calls = {
        "workspace_bytes": lambda: lib.rss_flow_aggregate_workspace_bytes(a["n"], a["words"], a["out"]),
        "device": lambda: lib.rss_flow_aggregate_device(
            a["tuples"], a["words"], a["weights"], a["n"], a["flows"], a["loads"], a["first"],
            a["nflows"], a["ws"], a["ws_bytes"], None),
        "host": lambda: lib.rss_flow_aggregate_host(
            a["ctx"], a["tuples"], a["words"], a["weights"], a["n"], a["flows"], a["loads"],
            a["first"], ctypes.byref(size) if a["nflows"] else None)}
    for who in entries:
        assert calls[who]() == -22
        err = lib.rss_last_error().decode()
        assert err.startswith("rss_flow_aggregate_%s:" % who) and message in err, err


def test_workspace_bytes():
    """12 bytes per slot of the power of two >= 2n (at least 1024), slot_of and the tile counts
    (one per 1024 packets), each rounded to 8 bytes."""
    assert _native.flow_aggregate_workspace_bytes(4) == 1024 * 12 + 16 + 8
    assert _native.flow_aggregate_workspace_bytes(4099, 9) == 16384 * 12 + 16400 + 24


@pytest.mark.parametrize("argv,message", [
    (["--pcap", "b.pcap", "--aggregate"], "--aggregate folds the rows of a CSV"),
    (["--ips-file", "a.csv", "--ipv6", "--aggregate"], "IPv4 flows only")])
def test_cli_flags(argv, message, capsys):
    with pytest.raises(SystemExit) as stop:
        keysearch.main(argv + ["--htable-size", "128", "--num-queues", "24"])
    err = capsys.readouterr().err
    assert stop.value.code == 2 and re.search(message, err), err
