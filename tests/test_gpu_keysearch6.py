"""GPU parity for key search over IPv6 tuples: every row of rss_key_search6_device and all 320
rows of rss_key_neighbourhood6_device == the oracle's counts (oracle_run_words, the literal
rotating-key loop), across modulo modes, every bin tier of the two launchers and misaligned
input; and the --ipv6 command line on top of them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def native():
    from rss_simulator_nvidia_amd import _native
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a gfx950 device")
    return _native


def words(seed, n):
    return np.random.RandomState(seed).randint(0, 2**32, (n, 9), dtype=np.uint32)


def oracle_counts(oracle_lib, key, tuples, H, Q):
    return oracle_lib.run_words(key, tuples, H, Q)[2][:min(H, Q)]


def keys11(seed):
    """11 keys (the last 8-, 4- and 2-key group is partial) of 40 and 52 bytes."""
    from rss_simulator_nvidia_amd import keysearch
    return [keysearch.random_keys(1, seed=seed + i, length=40 if i % 2 == 0 else 52)[0]
            for i in range(11)]


@pytest.mark.parametrize("H,Q,n", [
    (128, 24, 2003), (128, 24, 0), (128, 24, 3), (1, 1, 2003), (100, 7, 2003), (16, 24, 2003),
    (128, 16, 2003), (512, 64, 2003), (65536, 24, 2003), (131072, 24, 2003), (100000, 7, 2003),
    # kBins6BytesMax = 147712 B of bins: 8 keys per workgroup up to 144 queues, 4 up to 288 ...
    (256, 144, 2003), (256, 145, 2003), (1024, 288, 2003), (1024, 289, 2003),
    # ... pairs with lane-private bins up to 577, shared bins up to 18464 ...
    (1024, 577, 2003), (1024, 578, 2003), (1000, 578, 2003), (32768, 18464, 2003),
    # ... and global atomics past them
    (32768, 18465, 2003), (100000, 20000, 2003)])
def test_every_key_matches_oracle(native, oracle_lib, H, Q, n):
    from rss_simulator_nvidia_amd import keysearch
    keys, tuples = keys11(H + Q), words(H * 7 + n, n)
    counts = keysearch.evaluate(keys, tuples, H, Q, ipv6=True)
    assert counts.shape == (11, min(H, Q))
    np.testing.assert_array_equal(
        counts, np.stack([oracle_counts(oracle_lib, k, tuples, H, Q) for k in keys]))


def test_identical_tuples_and_a_field_selected_key(native, oracle_lib, example_key):
    """Every add of a key on one queue; and a key of the addresses only is just other windows:
    the oracle over the tuple's eight address words."""
    H, Q = 128, 24
    same = np.repeat(words(9, 1), 2003, axis=0)
    tuples = words(10, 2003)
    ctx = native.HostContext(0)
    keys = [native.prepare_key6(example_key, native.FIELDS_IP), native.prepare_key6(example_key)]
    got = ctx.key_search6(keys, same, H, Q)
    np.testing.assert_array_equal(got[1], oracle_counts(oracle_lib, example_key, same, H, Q))
    assert got[1].max() == 2003
    got = ctx.key_search6(keys, tuples, H, Q)
    np.testing.assert_array_equal(got[0], oracle_counts(oracle_lib, example_key, tuples[:, :8], H, Q))
    np.testing.assert_array_equal(got[1], oracle_counts(oracle_lib, example_key, tuples, H, Q))


def oracle_rows(oracle_lib, key, tuples, H, Q, rows=range(320)):
    from rss_simulator_nvidia_amd import keysearch
    return np.stack([oracle_counts(oracle_lib, keysearch.flip_bit(key, j), tuples, H, Q)
                     for j in rows])


@pytest.mark.parametrize("H,Q,n", [
    (128, 24, 2003), (128, 24, 0), (128, 24, 5), (1, 1, 2003), (100, 7, 2003), (16, 24, 2003),
    (100000, 7, 2003), (65536, 1000, 2003),
    # kNbr6BinBytesMax = 155776 B of bins: lane-private, 32 / 16 / 8 / 4 / 2 / 1 neighbours per
    # workgroup ...
    (256, 38, 2003), (256, 39, 2003), (256, 76, 2003), (256, 77, 2003), (1000, 152, 2003),
    (1024, 153, 2003), (1024, 304, 2003), (1000, 305, 2003), (4096, 608, 2003),
    (4096, 609, 2003), (4096, 1217, 2003),
    # ... shared bins, 16 / 8 / 4 / 2 / 1 ...
    (4096, 1218, 2003), (4096, 2434, 2003), (4096, 2435, 2003), (8192, 4868, 2003),
    (70000, 4869, 2003), (16384, 9736, 2003), (16384, 9737, 2003), (32768, 19472, 2003),
    (32768, 19473, 2003), (65536, 38944, 2003),
    # ... and global atomics past them
    (65536, 38945, 2003), (100000, 45000, 2003)])
def test_every_neighbour_matches_oracle(native, oracle_lib, H, Q, n):
    from rss_simulator_nvidia_amd import keysearch
    key = keysearch.random_keys(1, seed=H + Q, length=40 if Q % 2 else 52)[0]
    tuples = words(H * 7 + n, n)
    counts = keysearch.neighbourhood(key, tuples, H, Q, ipv6=True)
    assert counts.shape == (320, min(H, Q))
    np.testing.assert_array_equal(counts, oracle_rows(oracle_lib, key, tuples, H, Q))


@pytest.mark.parametrize("entry", ["search6", "neighbourhood6"])
def test_device_api_misaligned(native, oracle_lib, example_key, entry):
    from rss_simulator_nvidia_amd import keysearch
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream
    n, H, Q = 2003, 128, 24
    host = words(777, n)
    shifted = torch.empty(9 * n + 1, dtype=torch.int32, device=dev)
    shifted[1:] = torch.from_numpy(host.view(np.int32).reshape(-1)).to(dev)
    assert shifted[1:].data_ptr() % 16 == 4 and n % 4
    counts = torch.full((320, Q), 5, dtype=torch.int64, device=dev)
    if entry == "search6":  # the same job as a search over the 320 host-prepared flipped keys
        win = np.stack([np.ctypeslib.as_array(native.prepare_key6(keysearch.flip_bit(example_key, j)).window)
                        for j in range(320)]).astype(np.uint32)
        windows = torch.from_numpy(win.view(np.int32)).to(dev)
        native.key_search6_device(windows.data_ptr(), 320, shifted[1:].data_ptr(), n, H, Q,
                                  counts.data_ptr(), s)
    else:
        native.key_neighbourhood6_device(native.prepare_key6(example_key), shifted[1:].data_ptr(),
                                         n, H, Q, counts.data_ptr(), s)
    torch.cuda.synchronize()
    got = counts.cpu().numpy().view(np.uint64)
    rows = (0, 160, 318, 319)
    np.testing.assert_array_equal(got[list(rows)], oracle_rows(oracle_lib, example_key, host, H, Q, rows))
    np.testing.assert_array_equal(got[319], oracle_counts(oracle_lib, example_key, host, H, Q))
    assert (got.sum(axis=1) == n).all()


def test_cli_ipv6_refine_writes_the_best_key(native, oracle_lib, tmp_path):
    import ipaddress
    from rss_simulator_nvidia_amd import keysearch
    w = words(42, 600)
    addr = lambda r: str(ipaddress.IPv6Address(b"".join(int(x).to_bytes(4, "big") for x in r)))  # noqa: E731
    ips = tmp_path / "ips6.csv"
    ips.write_text("src_ip,dst_ip,src_port,dst_port\n" + "".join(
        "%s,%s,%d,%d\n" % (addr(r[0:4]), addr(r[4:8]), r[8] >> 16, r[8] & 0xFFFF) for r in w))
    out = tmp_path / "best.txt"
    ranked = keysearch.main(["--ipv6", "--ips-file", str(ips), "--htable-size", "128",
                             "--num-queues", "24", "--keys", "16", "--refine", "3",
                             "--out", str(out)])
    tuples = np.ascontiguousarray(keysearch.load_tuples(str(ips), ipv6=True)).view(np.uint32).reshape(-1, 9)
    np.testing.assert_array_equal(tuples, w)
    assert len(ranked) == 1 + 5 and out.read_text() == keysearch.key_text(ranked[0]["key"])
    assert len(ranked[0]["flips"]) <= 3
    for r in ranked:
        np.testing.assert_array_equal(r["counts"], oracle_counts(oracle_lib, r["key"], tuples, 128, 24))
    assert (ranked[0]["max_load"], ranked[0]["chi2"]) <= (ranked[1]["max_load"], ranked[1]["chi2"])
