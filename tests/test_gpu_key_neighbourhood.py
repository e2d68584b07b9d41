"""GPU parity for the key neighbourhood: each of the 128 single-bit-flip rows == the oracle's
counts for the flipped key, across modulo modes, every bin tier of the launcher and
misaligned input; and the hill climb on top of it."""
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


def oracle_rows(oracle_lib, key, tuples, H, Q, rows=range(128)):
    from rss_simulator_nvidia_amd import keysearch
    return [oracle_lib.run(keysearch.flip_bit(key, j), tuples, H, Q)[2][:min(H, Q)] for j in rows]


@pytest.mark.parametrize("H,Q,n,klen", [
    (128, 24, 4099, 40), (128, 24, 0, 40), (1, 1, 5, 40), (100, 7, 4097, 52), (16, 24, 3333, 16),
    (100000, 7, 2001, 40), (65536, 1000, 3001, 40),
    # both sides of every bin-budget edge: lane-private bins, 32 / 16 / 8 / 4 / 2 / 1
    # neighbours per workgroup ...
    (256, 39, 2003, 40), (256, 40, 2003, 40), (256, 78, 2003, 40), (256, 79, 2003, 40),
    (1000, 157, 2003, 40), (1024, 158, 2003, 40), (1024, 314, 2003, 40), (1000, 315, 2003, 40),
    (4096, 629, 2003, 40), (4096, 630, 2003, 40), (4096, 1259, 2003, 40),
    # ... shared bins, 16 / 8 / 4 / 2 / 1 ...
    (4096, 1260, 2003, 40), (4096, 2518, 2003, 40), (4096, 2519, 2003, 40),
    (8192, 5036, 2003, 40), (70000, 5037, 2003, 40), (16384, 10072, 2003, 40),
    (16384, 10073, 2003, 40), (32768, 20144, 2003, 40), (32768, 20145, 2003, 40),
    (65536, 40288, 2003, 40),
    # ... and global atomics past them
    (65536, 40289, 2003, 40), (100000, 45000, 1999, 40)])
def test_every_row_matches_oracle(native, oracle_lib, H, Q, n, klen):
    from rss_simulator_nvidia_amd import keysearch
    key = keysearch.random_keys(1, seed=H + Q, length=klen)[0]
    tuples = oracle_lib.generate(H * 7 + n, 0, n)
    counts = keysearch.neighbourhood(key, tuples, H, Q)
    assert counts.shape == (128, min(H, Q))
    np.testing.assert_array_equal(counts, np.stack(oracle_rows(oracle_lib, key, tuples, H, Q)))


def test_device_api_misaligned_flow_input(native, oracle_lib, example_key):
    import bench
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream
    n, H, Q = 50021, 128, 24
    host = bench.flow_np(777, n)
    shifted = torch.empty(3 * n + 1, dtype=torch.int32, device=dev)
    shifted[1:] = torch.from_numpy(host.view(np.int32).reshape(-1)).to(dev)
    assert shifted[1:].data_ptr() % 16 == 4 and n % 4
    counts = torch.full((128, Q), 5, dtype=torch.int64, device=dev)
    native.key_neighbourhood_device(native.prepare_key(example_key), shifted[1:].data_ptr(), n, H,
                                    Q, counts.data_ptr(), s)
    torch.cuda.synchronize()
    got = counts.cpu().numpy().view(np.uint64)
    rows = (0, 64, 126, 127)
    np.testing.assert_array_equal(got[list(rows)],
                                  np.stack(oracle_rows(oracle_lib, example_key, host, H, Q, rows)))
    assert (got.sum(axis=1) == n).all()


def test_cli_refine_writes_the_best_refined_key(native, oracle_lib, golden_dir, tmp_path):
    import os
    from rss_simulator_nvidia_amd import keysearch
    ips = os.path.join(golden_dir, "example_input", "ips.csv")
    out = tmp_path / "best.txt"
    ranked = keysearch.main(["--ips-file", ips, "--htable-size", "128", "--num-queues", "24",
                             "--keys", "16", "--refine", "3", "--out", str(out), "--key-file",
                             os.path.join(golden_dir, "example_input", "hash_key.txt")])
    assert len(ranked) == 2 + 5 and out.read_text() == keysearch.key_text(ranked[0]["key"])
    tuples = np.ascontiguousarray(keysearch.load_tuples(ips)).view(np.uint32).reshape(-1, 3)
    for r in ranked[:2]:  # the refined keys, best first, each no worse than any ranked start
        assert len(r["flips"]) <= 3
        np.testing.assert_array_equal(r["counts"], oracle_lib.run(r["key"], tuples, 128, 24)[2])
    assert (ranked[0]["max_load"], ranked[0]["chi2"]) <= (ranked[1]["max_load"], ranked[1]["chi2"])
    assert (ranked[0]["max_load"], ranked[0]["chi2"]) <= (ranked[2]["max_load"], ranked[2]["chi2"])


def test_refine_end_to_end_improves_on_example_key(native, oracle_lib, example_key):
    from rss_simulator_nvidia_amd import keysearch
    tuples = oracle_lib.generate(11, 0, 200000)
    base = keysearch.balance(oracle_lib.run(example_key, tuples, 128, 24)[2], 128, 24)
    r = keysearch.refine(example_key, tuples, 128, 24)
    assert (r["max_load"], r["chi2"]) < (base["max_load"][0], base["chi2"][0])
    np.testing.assert_array_equal(r["counts"], oracle_lib.run(r["key"], tuples, 128, 24)[2])
