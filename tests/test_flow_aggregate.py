"""Flow aggregation without a GPU: every entry's argument validation (refused before any device
work), the workspace size, the CLI's flags, and the table's hash: the header the kernel includes,
compiled for the host, against the numpy port and pre-images (flow_hash.py) from which the GPU
suite builds its forced collisions."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flow_hash
from rss_simulator_nvidia_amd import _native, keysearch

PTR = 0x1000  # never dereferenced: validation comes first
BIG = (1 << 30) + 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def header_hash(tmp_path_factory):
    """hashes(tuples) by tests/native/flow_hash_main.cpp, which includes only rss_flow_hash.h."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    work = tmp_path_factory.mktemp("flow_hash")
    exe = str(work / "flow_hash_main")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "rss_simulator_nvidia_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "native", "flow_hash_main.cpp")], check=True)

    def hashes(tuples):
        path = work / "tuples.bin"
        path.write_bytes(np.ascontiguousarray(tuples, dtype="<u4").tobytes())
        out = subprocess.run([exe, str(tuples.shape[1]), str(path)], check=True,
                             capture_output=True, text=True).stdout
        return np.array([int(line, 16) for line in out.split()], dtype=np.uint32)
    return hashes


@pytest.mark.parametrize("words", [3, 9])
def test_hash_port_and_preimage_match_the_header(header_hash, words):
    rng = np.random.default_rng(words)
    tuples = rng.integers(0, 2**32, (4000, words), dtype=np.uint64).astype(np.uint32)
    tuples[0], tuples[1] = 0, 0xFFFFFFFF
    np.testing.assert_array_equal(flow_hash.agg_hash(tuples), header_hash(tuples))
    # pre-images: one target for all rows (the last slot of both tables), and a target per row
    ones = flow_hash.preimage(tuples[:, :words - 1], 0xFFFFFFFF)
    targets = rng.integers(0, 2**32, 4000, dtype=np.uint64).astype(np.uint32)
    targets[:3] = 0, 1, 0xFFFFFFFE
    each = flow_hash.preimage(tuples[:, :words - 1], targets)
    for rows, want in ((ones, np.full(4000, 0xFFFFFFFF, np.uint32)), (each, targets)):
        assert rows.dtype == np.uint32 and rows.shape == (4000, words)
        np.testing.assert_array_equal(rows[:, :words - 1], tuples[:, :words - 1])
        np.testing.assert_array_equal(header_hash(rows), want)
        np.testing.assert_array_equal(flow_hash.agg_hash(rows), want)
        assert len(np.unique(rows, axis=0)) == 4000
    nslots = 2 * flow_hash.CHUNK[words]
    assert flow_hash.local_slot(0xFFFFFFFF, words) == nslots - 1
    for local, global_, cap in ((nslots - 2, 4093, 4096), (0, 0, 4096), (1, 1, 4096), (nslots - 1, 5, 1024)):
        h = flow_hash.hash_for_slots(local, global_, words, cap)
        assert flow_hash.local_slot(h, words) == local and h % cap == global_


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
