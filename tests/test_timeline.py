"""Key search over time without a GPU: the peak of hand-made loads, the windows of a time
column, every refusal of the Python layer and the command line, and the C entries' argument
validation (refused before any device work)."""
import re

import numpy as np
import pytest

from rss_simulator_nvidia_amd import _native, keysearch

PTR = 0x1000  # never dereferenced: validation comes first


def test_peak_of_hand_made_loads():
    share = keysearch.slot_share(128, 24)  # 6 buckets for queues 0..7, 5 for the rest
    level = np.round(share * 128 * 10)     # a perfectly level window of 1280
    quiet = level / 10                     # a tenth of it, level too
    hot = quiet.copy()
    hot[9] = level[9] * 2                  # a quiet window with one queue at twice the level one's
    one = keysearch.peak(np.stack([quiet, level, quiet]), 128, 24)
    assert one["peak"][0] == pytest.approx(1.0) and one["window"][0] == 1
    two = keysearch.peak(np.stack([np.stack([quiet, level, quiet]), np.stack([level, quiet, hot])]),
                         128, 24)
    assert two["peak"][1] == pytest.approx(2.0) and list(two["window"]) == [1, 2]
    # Q > H: the rows are H wide and every queue owns one bucket
    wide = keysearch.peak(np.array([[4, 0, 0, 0], [1, 1, 1, 1]]), 4, 9)
    assert wide["peak"][0] == pytest.approx(4.0) and wide["window"][0] == 0
    assert keysearch.peak(np.zeros((2, 3, 24)), 128, 24)["peak"].tolist() == [0.0, 0.0]


def test_window_slots_from_a_time_column():
    slots, nslots = keysearch.window_slots(np.array([10.0, 10.49, 10.5, 12.0, 9.5, 11.99]), 0.5)
    assert slots.dtype == np.uint32 and list(slots) == [1, 1, 2, 5, 0, 4] and nslots == 6
    slots, nslots = keysearch.window_slots(np.array([7, 7, 7]), 1000)
    assert list(slots) == [0, 0, 0] and nslots == 1
    assert keysearch.window_slots(np.array([], dtype=np.int64), 1)[1] == 1


@pytest.mark.parametrize("call,error,message", [
    (lambda: keysearch.window_slots(np.array([1.0, 2.0]), 0), ValueError, "must be > 0"),
    (lambda: keysearch.window_slots(np.array([1.0, 2.0]), -1.5), ValueError, "must be > 0"),
    (lambda: keysearch.window_slots(np.array(["a", "b"]), 1), ValueError, "one number per packet"),
    (lambda: keysearch.window_slots(np.array([1.0, np.nan]), 1), ValueError, "finite"),
    (lambda: keysearch.window_slots(np.array([0.0, 1e12]), 1), ValueError, r"more than 2\^32"),
    (lambda: keysearch.timeline([list(range(40))], np.zeros((2, 9), np.uint32), [0, 0], 128, 24,
                                ipv6=True), NotImplementedError, "IPv4 tuples only"),
    (lambda: keysearch.timeline([list(range(40))], np.zeros((4, 3), np.uint32), [0, 1, 2], 128,
                                24), ValueError, "one slot per packet"),
    (lambda: _native.tuple_slots(np.array([0, 1, -1, 2]), 4), ValueError, r"\[0, 2\^32\)"),
    (lambda: _native.tuple_slots(np.array([0, 1, 2**32, 2]), 4), ValueError, r"\[0, 2\^32\)"),
    (lambda: _native.tuple_slots(np.array([0.0, 1.0, 1.5, 2.0]), 4), ValueError, "integers"),
    (lambda: keysearch.timeline([list(range(40))], np.zeros((1, 3), np.uint32), [0], 128, 24,
                                nslots=0), ValueError, "nslots")])
def test_python_layer_refusals(call, error, message):
    with pytest.raises(error, match=message):
        call()


@pytest.mark.parametrize("argv,message", [
    (["--ips-file", "CSV", "--time-column", "t"], "--time-column and --window go together"),
    (["--ips-file", "CSV", "--window", "1"], "--time-column and --window go together"),
    (["--pcap", "b.pcap", "--time-column", "t", "--window", "1"], "cannot be combined with --pcap"),
    (["--ips-file", "CSV", "--ipv6", "--time-column", "t", "--window", "1"],
     "cannot be combined with --pcap, --ipv6"),
    (["--ips-file", "CSV", "--aggregate", "--time-column", "t", "--window", "1"],
     "cannot be combined with --pcap, --ipv6 or --aggregate"),
    (["--ips-file", "CSV", "--time-column", "nope", "--window", "1"], "has no column 'nope'"),
    (["--ips-file", "CSV", "--time-column", "when", "--window", "1"], "is not numeric"),
    (["--ips-file", "CSV", "--time-column", "t", "--window", "1", "--weight-column", "nope"],
     "has no column 'nope'"),
    (["--ips-file", "CSV", "--time-column", "t", "--window", "0"], "--window must be > 0"),
    (["--ips-file", "CSV", "--time-column", "t", "--window", "-2"], "--window must be > 0"),
    (["--ips-file", "CSV", "--time-column", "t", "--window", "wide"], "invalid float value")])
def test_cli_refusals(argv, message, tmp_path, capsys):
    csv = tmp_path / "packets.csv"
    csv.write_text("src_ip,dst_ip,src_port,dst_port,t,when\n1.1.1.1,2.2.2.2,1,2,0.5,noon\n")
    argv = [str(csv) if a == "CSV" else a for a in argv]
    with pytest.raises(SystemExit) as stop:
        keysearch.main(argv + ["--htable-size", "128", "--num-queues", "24"])
    err = capsys.readouterr().err
    assert stop.value.code == 2 and err.startswith("usage: rss-keysearch")
    assert re.search(message, err), err


@pytest.mark.parametrize("change,message", [
    (dict(keys=None), "or loads is NULL"), (dict(loads=None), "or loads is NULL"),
    (dict(slots=None), "slots is NULL"), (dict(nkeys=0), "no keys"), (dict(nslots=0), "no slots"),
    (dict(tuples=None), "tuples is NULL"), (dict(H=0), "must be >= 1"), (dict(Q=0), "must be >= 1")])
def test_validation_before_any_device_work(change, message):
    lib = _native.load()
    a = dict(keys=PTR, nkeys=2, tuples=PTR, weights=None, slots=PTR, n=4, nslots=3, H=128, Q=24,
             loads=PTR)
    a.update(change)
    args = (a["keys"], a["nkeys"], a["tuples"], a["weights"], a["slots"], a["n"], a["nslots"],
            a["H"], a["Q"], a["loads"])
    for who, call in (("device", lambda: lib.rss_key_search_timeline_device(*args, None)),
                      ("host", lambda: lib.rss_key_search_timeline_host(PTR, *args))):
        assert call() == -22
        err = lib.rss_last_error().decode()
        assert err.startswith("rss_key_search_timeline_%s:" % who) and message in err, err
