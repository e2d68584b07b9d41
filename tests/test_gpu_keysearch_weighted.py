"""GPU parity for key search by load: rss_key_search_weighted_* and
rss_key_neighbourhood_weighted_* against exact per-queue sums of the weights over the oracle's
queues, on each side of every bin tier of the two launchers, with weights that wrap a 32-bit
bin after two tuples; misaligned device input, graph replay, and the hill climb on loads."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROWS = (0, 64, 126, 127)


@pytest.fixture(scope="module")
def native():
    from rss_simulator_nvidia_amd import _native
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a gfx950 device")
    return _native


def loads_of(oracle_lib, keys, tuples, weights, H, Q):
    """Exact uint64 loads [len(keys), min(H, Q)]: the weights summed per oracle queue."""
    out = np.zeros((len(keys), min(H, Q)), dtype=np.uint64)
    for row, key in zip(out, keys):
        if len(tuples):
            np.add.at(row, oracle_lib.run(key, tuples, H, Q)[1], weights.astype(np.uint64))
    return out


def make_weights(kind, n, seed):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    return np.full(n, {"max": 0xFFFFFFFF, "zero": 0, "ones": 1}[kind], dtype=np.uint32)


@pytest.mark.parametrize("H,Q,n,nkeys,kind", [
    (128, 24, 4099, 11, "random"), (128, 24, 4099, 11, "ones"), (128, 24, 4099, 8, "zero"),
    (128, 24, 5, 3, "max"), (1, 1, 5, 3, "max"), (128, 24, 0, 5, "random"),
    # packed tables: 8 keys per workgroup to Q = 77, 4 to Q = 154, then pairs ...
    (256, 77, 2003, 11, "random"), (256, 78, 2003, 11, "random"), (1024, 154, 2003, 11, "random"),
    (1024, 155, 2003, 11, "random"), (131072, 24, 2001, 4, "random"),
    # ... pair tables (any H): private bins to Q = 80, shared to 2560, then global atomics
    (100, 7, 4097, 11, "ones"), (100, 80, 2003, 11, "random"), (1000, 81, 2003, 11, "random"),
    (4096, 2560, 2003, 5, "random"), (4096, 2561, 2003, 5, "random"),
    (100000, 45000, 1999, 3, "max")])
def test_search_loads_match_reference(native, oracle_lib, H, Q, n, nkeys, kind):
    from rss_simulator_nvidia_amd import keysearch
    keys = keysearch.random_keys(nkeys, seed=H + Q)
    tuples = oracle_lib.generate(H * 7 + n, 0, n)
    weights = make_weights(kind, n, Q)
    loads = keysearch.evaluate(keys, tuples, H, Q, weights=weights)
    assert loads.shape == (nkeys, min(H, Q)) and loads.dtype == np.uint64
    np.testing.assert_array_equal(loads, loads_of(oracle_lib, keys, tuples, weights, H, Q))
    if kind == "ones":
        np.testing.assert_array_equal(loads, keysearch.evaluate(keys, tuples, H, Q))


@pytest.mark.parametrize("H,Q,n,kind", [
    (128, 24, 4099, "random"), (128, 24, 4099, "ones"), (128, 24, 1001, "zero"),
    (128, 24, 5, "max"), (1, 1, 5, "max"), (128, 24, 0, "random"), (100, 7, 4097, "random"),
    # lane-private bins, 32 / 16 / 8 / 4 / 2 / 1 neighbours per workgroup ...
    (256, 19, 1003, "random"), (256, 20, 1003, "random"), (256, 39, 1003, "random"),
    (256, 40, 1003, "random"), (256, 78, 1003, "random"), (1000, 79, 1003, "random"),
    (1024, 157, 1003, "random"), (1024, 158, 1003, "random"), (1024, 314, 1003, "random"),
    (1000, 315, 1003, "random"), (4096, 629, 1003, "random"),
    # ... shared bins, 16 / 8 / 4 / 2 / 1 ...
    (4096, 630, 1003, "random"), (4096, 1259, 1003, "random"), (4096, 1260, 1003, "random"),
    (4096, 2518, 1003, "random"), (4096, 2519, 1003, "random"), (8192, 5036, 1003, "random"),
    (70000, 5037, 1003, "random"), (16384, 10072, 1003, "random"),
    (16384, 10073, 1003, "random"), (32768, 20144, 1003, "random"),
    # ... and global atomics past them
    (32768, 20145, 1003, "random"), (100000, 45000, 999, "max")])
def test_neighbourhood_loads_match_reference(native, oracle_lib, H, Q, n, kind):
    from rss_simulator_nvidia_amd import keysearch
    key = keysearch.random_keys(1, seed=H + Q)[0]
    tuples = oracle_lib.generate(H * 7 + n, 0, n)
    weights = make_weights(kind, n, H)
    loads = keysearch.neighbourhood(key, tuples, H, Q, weights=weights)
    assert loads.shape == (128, min(H, Q))
    flips = [keysearch.flip_bit(key, j) for j in range(128)]
    np.testing.assert_array_equal(loads, loads_of(oracle_lib, flips, tuples, weights, H, Q))
    if kind == "ones":
        np.testing.assert_array_equal(loads, keysearch.neighbourhood(key, tuples, H, Q))


def test_device_api_misaligned_input_and_stale_output(native, oracle_lib, example_key):
    """Tuples and weights both at a pointer = 4 mod 16 (the one-tuple-per-lane body) and the
    loads pre-filled with garbage (the clearing kernel), for both entries."""
    from rss_simulator_nvidia_amd import keysearch
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream
    n, H, Q = 5003, 128, 24
    host = oracle_lib.generate(777, 0, n)
    weights = make_weights("random", n, 3)
    d_t = torch.empty(3 * n + 1, dtype=torch.int32, device=dev)
    d_w = torch.empty(n + 1, dtype=torch.int32, device=dev)
    d_t[1:] = torch.from_numpy(host.view(np.int32).reshape(-1)).to(dev)
    d_w[1:] = torch.from_numpy(weights.view(np.int32)).to(dev)
    assert d_t[1:].data_ptr() % 16 == 4 and d_w[1:].data_ptr() % 16 == 4 and n % 4
    keys = [keysearch.flip_bit(example_key, j) for j in ROWS]
    want = loads_of(oracle_lib, keys, host, weights, H, Q)
    nbr = torch.full((128, Q), 5, dtype=torch.int64, device=dev)
    native.key_neighbourhood_weighted_device(native.prepare_key(example_key), d_t[1:].data_ptr(),
                                             d_w[1:].data_ptr(), n, H, Q, nbr.data_ptr(), s)
    win = np.stack([np.ctypeslib.as_array(native.prepare_key(k).window) for k in keys])
    d_win = torch.from_numpy(win.astype(np.uint32).view(np.int32)).to(dev)
    found = torch.full((len(keys), Q), -7, dtype=torch.int64, device=dev)
    native.key_search_weighted_device(d_win.data_ptr(), len(keys), d_t[1:].data_ptr(),
                                      d_w[1:].data_ptr(), n, H, Q, found.data_ptr(), s)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(nbr.cpu().numpy().view(np.uint64)[list(ROWS)], want)
    np.testing.assert_array_equal(found.cpu().numpy().view(np.uint64), want)
    assert (nbr.cpu().numpy().view(np.uint64).sum(axis=1) == weights.sum(dtype=np.uint64)).all()


def test_graph_replay_follows_the_weights(native, oracle_lib, example_key):
    """The captured neighbourhood call clears its loads itself: each replay gives the loads
    of the weights then in the buffer, over whatever the loads held before."""
    from rss_simulator_nvidia_amd import keysearch
    dev = torch.device("cuda:0")
    n, H, Q = 4099, 128, 24
    host = oracle_lib.generate(21, 0, n)
    d_t = torch.from_numpy(host.view(np.int32).reshape(-1)).to(dev)
    d_w = torch.zeros(n, dtype=torch.int32, device=dev)
    loads = torch.empty((128, Q), dtype=torch.int64, device=dev)
    key = native.prepare_key(example_key)
    call = lambda: native.key_neighbourhood_weighted_device(  # noqa: E731
        key, d_t.data_ptr(), d_w.data_ptr(), n, H, Q, loads.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    call()  # eager first: code objects loaded before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            call()
    torch.cuda.current_stream().wait_stream(side)
    keys = [keysearch.flip_bit(example_key, j) for j in ROWS]
    for kind in ("random", "max", "random"):
        weights = make_weights(kind, n, 9)
        d_w.copy_(torch.from_numpy(weights.view(np.int32)))
        loads.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(loads.cpu().numpy().view(np.uint64)[list(ROWS)],
                                      loads_of(oracle_lib, keys, host, weights, H, Q))


def test_refine_on_loads_improves_on_example_key(native, oracle_lib, example_key):
    from rss_simulator_nvidia_amd import keysearch
    H, Q = 128, 24
    tuples = oracle_lib.generate(11, 0, 200000)
    weights = np.minimum(np.random.default_rng(5).zipf(1.3, len(tuples)), 0xFFFFFFFF).astype(np.uint32)
    base = keysearch.balance(loads_of(oracle_lib, [example_key], tuples, weights, H, Q), H, Q)
    r = keysearch.refine(example_key, tuples, H, Q, weights=weights)
    assert r["flips"] and (r["max_load"], r["chi2"]) < (base["max_load"][0], base["chi2"][0])
    np.testing.assert_array_equal(r["counts"],
                                  loads_of(oracle_lib, [r["key"]], tuples, weights, H, Q)[0])
