"""GPU parity for the byte neighbourhood: rows of rss_key_byte_neighbourhood_* == the oracle's
counts (loads: the weights summed per oracle queue) under the literally modified key, for all
bytes, on each side of every bin tier, from misaligned device input, and through the CLI."""
import os

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


def make_tuples(oracle_lib, seed, n, ipv6):
    if not ipv6:
        return oracle_lib.generate(seed, 0, n)
    return np.random.default_rng(seed).integers(0, 2**32, (n, 9), dtype=np.uint64).astype(np.uint32)


def reference(oracle_lib, key, rows, tuples, H, Q, ipv6=False, weights=None, first=0):
    """Rows ``rows`` (256 * (B - first) + v) of the byte neighbourhood from the oracle."""
    out = []
    for r in rows:
        k = list(key)
        k[first + (r >> 8)] = r & 0xFF
        _, queues, counts = (oracle_lib.run_words if ipv6 else oracle_lib.run)(k, tuples, H, Q)
        if weights is not None:  # sums stay below 2^53
            counts = np.bincount(queues, weights=weights.astype(np.float64), minlength=Q)
        out.append(counts[:min(H, Q)].astype(np.uint64))
    return np.stack(out)


@pytest.mark.parametrize("H,Q,n,klen,ipv6", [
    (128, 24, 1501, 40, False), (1, 1, 1003, 16, False), (100, 7, 1501, 52, False),
    (16, 24, 1003, 40, False), (65536, 1000, 1501, 40, False), (128, 24, 0, 40, False),
    (128, 24, 1001, 40, True), (100, 7, 1003, 40, True)])
def test_all_bytes(native, oracle_lib, H, Q, n, klen, ipv6):
    from rss_simulator_nvidia_amd import keysearch
    key = keysearch.random_keys(1, seed=H + Q, length=klen)[0]
    tuples = make_tuples(oracle_lib, H * 7 + n, n, ipv6)
    nbytes = 40 if ipv6 else 16
    got = keysearch.byte_neighbourhood(key, tuples, H, Q, ipv6=ipv6)
    assert got.shape == (nbytes * 256, min(H, Q)) and got.dtype == np.uint64
    if n == 0:
        assert not got.any()
        return
    own = [256 * B + key[B] for B in range(nbytes)]
    np.testing.assert_array_equal(got[own], np.repeat(reference(oracle_lib, key, own[:1], tuples, H,
                                                                Q, ipv6), nbytes, axis=0))
    last = got[256 * (nbytes - 1):]
    np.testing.assert_array_equal(last, last[np.arange(256) ^ 1])  # the last key bit feeds no hash
    bits = [256 * (j >> 3) + (key[j >> 3] ^ (0x80 >> (j & 7))) for j in range(8 * nbytes)]
    np.testing.assert_array_equal(got[bits], keysearch.neighbourhood(key, tuples, H, Q, ipv6=ipv6))
    some = np.random.default_rng(n).integers(0, nbytes * 256, 48)
    np.testing.assert_array_equal(got[some], reference(oracle_lib, key, some, tuples, H, Q, ipv6))


# (kind, lane-private bins' last queue count with 32 / 16 / 8 / 4 / 2 / 1 values per workgroup,
# shared bins' with 16 / 8 / 4 / 2 / 1; one more queue is the next tier, global atomics at the end)
EDGES = {"v4": (39, 78, 157, 314, 629, 1259, 2518, 5036, 10072, 20144, 40288),
         "v6": (38, 76, 152, 304, 608, 1217, 2434, 4868, 9736, 19472, 38944),
         "weighted": (19, 39, 78, 157, 314, 629, 1259, 2518, 5036, 10072, 20144)}


@pytest.mark.parametrize("kind,Q,B", [(kind, edge + over, (5, (39 if kind == "v6" else 15))[i % 2])
                                      for kind, edges in EDGES.items()
                                      for i, edge in enumerate(edges) for over in (0, 1)])
def test_both_sides_of_every_bin_tier(native, oracle_lib, kind, Q, B):
    from rss_simulator_nvidia_amd import keysearch
    H = 256 if Q < 256 else (65536, 100000)[B == 5]  # FAST8; mask and FAST16 / FAST32 queue steps
    n, ipv6 = 1003, kind == "v6"
    key = keysearch.random_keys(1, seed=Q)[0]
    tuples = make_tuples(oracle_lib, Q, n, ipv6)
    weights = None
    if kind == "weighted":
        weights = np.random.default_rng(Q).integers(0, 2**20, n).astype(np.uint32)
    got = keysearch.byte_neighbourhood(key, tuples, H, Q, bytes=range(B, B + 1), ipv6=ipv6,
                                       weights=weights)
    assert got.shape == (256, Q)
    np.testing.assert_array_equal(got, reference(oracle_lib, key, range(256), tuples, H, Q, ipv6,
                                                 weights, first=B))


def test_weights_zero_and_max_are_summed_exactly(native, oracle_lib, example_key):
    from rss_simulator_nvidia_amd import keysearch
    H, Q, n, rows = 128, 24, 1003, (0, 1, 100, 255, 256 + 77, 4095)
    tuples = oracle_lib.generate(3, 0, n)
    weights = np.where(np.arange(n) % 3 == 0, 0, 0xFFFFFFFF).astype(np.uint32)
    got = keysearch.byte_neighbourhood(example_key, tuples, H, Q, weights=weights)
    for r in rows:
        k = list(example_key)
        k[r >> 8] = r & 0xFF
        want = [0] * Q
        for q, w in zip(oracle_lib.run(k, tuples, H, Q)[1].tolist(), weights.tolist()):
            want[q] += w
        assert got[r].tolist() == want


@pytest.mark.parametrize("kind", ["v4", "v6", "weighted"])
def test_device_api_misaligned_input_and_stale_output(native, oracle_lib, example_key, kind):
    """Tuples (and weights) at a pointer = 4 mod 16, n % 4 != 0, the output pre-filled."""
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream
    n, H, Q, ipv6 = 5003, 128, 24, kind == "v6"
    first, nbytes = (3, 13) if not ipv6 else (30, 10)
    host = make_tuples(oracle_lib, 777, n, ipv6)
    weights = np.random.default_rng(3).integers(0, 2**20, n).astype(np.uint32)
    d_t = torch.empty(host.size + 1, dtype=torch.int32, device=dev)
    d_w = torch.empty(n + 1, dtype=torch.int32, device=dev)
    d_t[1:] = torch.from_numpy(host.view(np.int32).reshape(-1)).to(dev)
    d_w[1:] = torch.from_numpy(weights.view(np.int32)).to(dev)
    assert d_t[1:].data_ptr() % 16 == 4 and d_w[1:].data_ptr() % 16 == 4 and n % 4
    out = torch.full((nbytes * 256, Q), 5, dtype=torch.int64, device=dev)
    if kind == "v4":
        native.key_byte_neighbourhood_device(native.prepare_key(example_key), first, nbytes,
                                             d_t[1:].data_ptr(), n, H, Q, out.data_ptr(), s)
    elif kind == "v6":
        native.key_byte_neighbourhood6_device(native.prepare_key6(example_key), first, nbytes,
                                              d_t[1:].data_ptr(), n, H, Q, out.data_ptr(), s)
    else:
        native.key_byte_neighbourhood_weighted_device(
            native.prepare_key(example_key), first, nbytes, d_t[1:].data_ptr(),
            d_w[1:].data_ptr(), n, H, Q, out.data_ptr(), s)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    rows = (0, 255, 256 * 2 + 128, 256 * (nbytes - 1) + 1, 256 * nbytes - 1)
    w = weights if kind == "weighted" else None
    np.testing.assert_array_equal(got[list(rows)], reference(oracle_lib, example_key, rows, host, H,
                                                             Q, ipv6, w, first=first))
    assert (got.sum(axis=1) == (weights.sum(dtype=np.uint64) if kind == "weighted" else n)).all()


def test_cli_refine_by_bytes_writes_the_best_refined_key(native, oracle_lib, golden_dir, tmp_path):
    from rss_simulator_nvidia_amd import keysearch
    ips = os.path.join(golden_dir, "example_input", "ips.csv")
    out = tmp_path / "best.txt"
    ranked = keysearch.main(["--ips-file", ips, "--htable-size", "128", "--num-queues", "24",
                             "--keys", "16", "--refine", "2", "--refine-step", "byte", "--out",
                             str(out)])
    assert len(ranked) == 1 + 5 and out.read_text() == keysearch.key_text(ranked[0]["key"])
    tuples = np.ascontiguousarray(keysearch.load_tuples(ips)).view(np.uint32).reshape(-1, 3)
    best = ranked[0]  # the refined key: at most two bytes away from the ranked start
    assert len(best["moves"]) <= 2 and best["flips"] == []
    assert sum(a != b for a, b in zip(best["key"], ranked[1]["key"])) <= 2
    np.testing.assert_array_equal(best["counts"], oracle_lib.run(best["key"], tuples, 128, 24)[2])
    assert (best["max_load"], best["chi2"]) <= (ranked[1]["max_load"], ranked[1]["chi2"])
