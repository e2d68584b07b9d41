"""Key search by backlog without a GPU: the C entries' argument validation (refused before any
device work), the ticks the Python layer accepts, the command line's flags and the workspace
size."""
import ctypes
import re

import numpy as np
import pytest

from rss_simulator_nvidia_amd import _native, keysearch

PTR = 0x1000  # never dereferenced: validation comes first
NEED = 8 + 2 * 24 * 32  # one segment of 4 packets: its two ticks, 2 keys x 24 queues x 4 x int64


@pytest.mark.parametrize("change,message,entries", [
    (dict(keys=None), "or peaks is NULL", "dh"), (dict(peaks=None), "or peaks is NULL", "dh"),
    (dict(ticks=None), "ticks is NULL", "dh"), (dict(nkeys=0), "no keys", "dh"),
    (dict(tuples=None), "tuples is NULL", "dh"), (dict(H=0), "must be >= 1", "dh"),
    (dict(Q=0), "must be >= 1", "dh"), (dict(drain=2**31), "drain 2147483648 must be below 2^31", "dh"),
    (dict(n=2**31), "n must be below 2^31", "dh"), (dict(H=5000, Q=4097), "exceeds the 4096 queues", "dh"),
    (dict(ws=None), "workspace NULL or not 8-byte aligned (%d bytes needed)" % NEED, "d"),
    (dict(ws=PTR + 4), "workspace NULL or not 8-byte aligned (%d bytes needed)" % NEED, "d"),
    (dict(ws_bytes=NEED - 1), "need %d" % NEED, "d"),
    (dict(keys="blank"), "key 1 not prepared", "h")])
def test_validation_before_any_device_work(change, message, entries):
    lib = _native.load()
    a = dict(keys=PTR, nkeys=2, tuples=PTR, weights=None, ticks=PTR, n=4, drain=3, H=128, Q=24,
             peaks=PTR, ws=PTR, ws_bytes=NEED)
    a.update(change)
    if a["keys"] == "blank":  # a prepared key, then one that never was
        blank = (_native.RssKey * 2)(_native.prepare_key(list(range(40))), _native.RssKey())
        a["keys"] = ctypes.addressof(blank)
    args = (a["keys"], a["nkeys"], a["tuples"], a["weights"], a["ticks"], a["n"], a["drain"],
            a["H"], a["Q"], a["peaks"])
    calls = {"d": ("device", lambda: lib.rss_key_search_backlog_device(*args, a["ws"],
                                                                       a["ws_bytes"], None)),
             "h": ("host", lambda: lib.rss_key_search_backlog_host(PTR, *args))}
    for entry in entries:
        who, call = calls[entry]
        assert call() == -22
        err = lib.rss_last_error().decode()
        assert err.startswith("rss_key_search_backlog_%s:" % who) and message in err, err


@pytest.mark.parametrize("call,message", [
    (lambda: _native.tuple_ticks(np.array([0, 5, 4, 9]), 4), "non-decreasing"),
    (lambda: _native.tuple_ticks(np.array([-1, 0, 1, 2]), 4), r"\[0, 2\^32\)"),
    (lambda: _native.tuple_ticks(np.array([0, 1, 2, 2**32]), 4), r"\[0, 2\^32\)"),
    (lambda: _native.tuple_ticks(np.array([0, 1, 2]), 4), "one tick per packet"),
    (lambda: _native.tuple_ticks(np.array([0.0, 1.0, 1.5, 2.0]), 4), "integers"),
    (lambda: keysearch.backlog([list(range(40))], np.zeros((2, 3), np.uint32), [0, 1], 2**31, 128,
                               24), r"drain must be an integer in \[0, 2\^31\)"),
    (lambda: keysearch.backlog([list(range(40))], np.zeros((2, 3), np.uint32), [0, 1], 1.5, 128,
                               24), r"drain must be an integer in \[0, 2\^31\)")])
def test_python_layer_refusals(call, message):
    with pytest.raises(ValueError, match=message):
        call()


def test_ticks_accepted():
    t = _native.tuple_ticks([3, 3, 7, 2**32 - 1], 4)
    assert t.dtype == np.uint32 and t.flags.c_contiguous and list(t) == [3, 3, 7, 2**32 - 1]
    assert len(_native.tuple_ticks(np.zeros(0, dtype=np.int64), 0)) == 0


@pytest.mark.parametrize("argv,message", [
    (["--time-column", "t", "--window", "1", "--drain", "5"], "--drain and --tick go together"),
    (["--time-column", "t", "--window", "1", "--tick", "0.5"], "--drain and --tick go together"),
    (["--drain", "5", "--tick", "0.5"], "--drain and --tick need --time-column"),
    (["--window", "1", "--drain", "5", "--tick", "0.5"], "--drain and --tick need --time-column"),
    (["--time-column", "t", "--window", "1", "--drain", "5", "--tick", "0"], "--tick must be > 0"),
    (["--time-column", "t", "--window", "1", "--drain", "-1", "--tick", "1"],
     r"--drain must be an integer in \[0, 2\^31\)"),
    (["--time-column", "t", "--window", "1", "--drain", str(2**31), "--tick", "1"],
     r"--drain must be an integer in \[0, 2\^31\)"),
    (["--time-column", "t", "--drain", "5", "--tick", "1"], "--time-column and --window go together")])
def test_cli_refusals(argv, message, tmp_path, capsys):
    csv = tmp_path / "packets.csv"
    csv.write_text("src_ip,dst_ip,src_port,dst_port,t\n1.1.1.1,2.2.2.2,1,2,0.5\n")
    with pytest.raises(SystemExit) as stop:
        keysearch.main(["--ips-file", str(csv), "--htable-size", "128", "--num-queues", "24"] + argv)
    err = capsys.readouterr().err
    assert stop.value.code == 2 and err.startswith("usage: rss-keysearch")
    assert re.search(message, err), err


def test_workspace_bytes_is_a_function_of_its_arguments():
    size = _native.key_search_backlog_workspace_bytes
    assert size(2, 4, 128, 24) == NEED
    assert size(2, 4, 16, 24) == 8 + 2 * 16 * 32  # min(H, Q) queues
    assert size(2, 0, 128, 24) > 0
    assert size(2, 10**6, 128, 24) > size(2, 10**4, 128, 24) > size(2, 4, 128, 24)
    assert size(64, 10**6, 128, 24) > size(8, 10**6, 128, 24)
    assert size(8, 2**31 - 1, 128, 24) == size(8, 2**30, 128, 24)  # the segments are capped
    lib = _native.load()
    assert lib.rss_key_search_backlog_workspace_bytes(2, 4, 128, 24, None) == -22
    assert lib.rss_last_error().decode().startswith("rss_key_search_backlog_workspace_bytes:")
