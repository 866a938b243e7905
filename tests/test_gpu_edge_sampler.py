"""The edge sampler and the edge counter of csrc/mde_edges.hip against the integer replay of
tests/_edges_reference.py: uniformity over the pairs for small requests, every returned edge one of the replayed
draws up to n = 2^31 - 1, ``mde_edges_count_unique`` through ctypes, and the refusal of items outside
``[0, n_items)`` at every door that forms the key ``min * n + max``."""
import ctypes
import time

import numpy as np
import pytest
import torch

import _edges_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the 1e-6 tails of chi-square with 52 and with 498 degrees of freedom: a correct sampler fails a case about once in
# a million runs (numpy's Generator.choice gives 37 .. 59 and 488 .. 510 on these shapes)
CHI2_52, CHI2_498 = 115.5, 662.7


def _sample_many(n, per_call, calls, exclude=None):
    from pymde_amd import preprocess
    ex = None if exclude is None else torch.as_tensor(exclude, device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = [preprocess.sample_edges(n, per_call, exclude=ex, seed=seed, device=DEV) for seed in range(calls)]
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    assert all(o.shape == (per_call, 2) for o in out)
    return torch.cat(out).cpu().numpy(), seconds


@pytest.mark.parametrize("n,per_call,calls,cells,excluded,bound", [
    (2000, 10, 1500, 53, 0, CHI2_52),
    (45, 10, 1500, 53, 0, CHI2_52),
    (45, 10, 1500, 53, 500, CHI2_52),
    (2000, 100, 600, 499, 0, CHI2_498),
], ids=["n2000-10", "n45-10", "n45-10-excl500", "n2000-100"])
def test_small_requests_are_uniform_over_the_pairs(n, per_call, calls, cells, excluded, bound):
    """``calls`` calls with seeds 0 .. calls - 1; the pair index of every sampled edge is binned into ``cells`` equal
    cells of the (i, j) order and compared with the exact number of eligible pairs of each cell.  Dropping a surplus
    at fixed ranks of the sorted keys, as the sampler did, leaves one edge near each fixed quantile: chi-square
    18 816.7, 26 204.4, 9 155.5 and 820.4 on these four cases on an MI355X, against 41.6, 49.4, 29.9 and 474.5 with
    the random thinning.  The calls of a case took 0.57 s, 0.34 s, 0.46 s and 0.15 s there."""
    exclude = None
    if excluded:
        exclude = np.array([ref.pair_of_index(n, i) for i in range(excluded)])
    edges, seconds = _sample_many(n, per_call, calls, exclude)
    assert (edges[:, 0] < edges[:, 1]).all() and edges.min() >= 0 and edges.max() < n
    chi2 = ref.cell_chi2(n, edges, cells, range(excluded))
    print(f"sample_edges n={n} {per_call} x {calls} calls, {excluded} excluded: chi2 = {chi2:.1f} over {cells} cells "
          f"(bound {bound}), {seconds:.2f} s")
    assert chi2 < bound, chi2
    # and the calls differ from each other: the seed matters (at n = 45 it hardly did)
    first = edges.reshape(calls, per_call, 2)
    assert len({first[c].tobytes() for c in range(calls)}) > 0.99 * calls


@pytest.mark.parametrize("n", [3, 60, 2 ** 26 + 3, 2 ** 30 + 7, 2 ** 31 - 1])
def test_every_returned_edge_is_a_replayed_draw(n):
    """No exclusion, 20 000 edges (C(n, 2) when that is fewer): the output is sorted, distinct, of the requested
    length and a subset of the host replay of the rounds' draws -- one round at the three large n, where
    ``4 n (n - 1)`` no longer fits a double exactly, and an enumeration of every pair at the two small ones.  This
    holds the index -> (u, v) map to the integer arithmetic bit for bit."""
    from pymde_amd import preprocess
    seed = 12345
    num = min(20000, ref.n_pairs(n))
    got = preprocess.sample_edges(n, num, seed=seed, device=DEV).cpu().numpy()
    assert got.shape == (num, 2)
    assert (got[:, 0] < got[:, 1]).all() and got.min() >= 0 and got.max() < n
    d = np.diff(got, axis=0)
    assert ((d[:, 0] > 0) | ((d[:, 0] == 0) & (d[:, 1] > 0))).all()          # sorted by (i, j) and distinct
    pairs, rounds = ref.replay(n, num, seed)
    assert rounds == 1
    if n <= 60:
        assert len(pairs) == num                                             # every pair there is
    missing = {tuple(e) for e in got.tolist()} - pairs
    assert not missing, sorted(missing)[:5]
    # the same call again gives the same edges, another seed others
    again = preprocess.sample_edges(n, num, seed=seed, device=DEV).cpu().numpy()
    np.testing.assert_array_equal(again, got)
    if n > 60:
        other = preprocess.sample_edges(n, num, seed=seed + 1, device=DEV).cpu().numpy()
        assert not np.array_equal(other, got)


def _count_unique(n, pairs):
    """``mde_edges_count_unique`` through ctypes: ``(rc, edges, weights)``."""
    from pymde_amd import _lib
    lib = _lib.load()
    p = len(pairs)
    dev = torch.as_tensor(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), device=DEV).contiguous()
    edges = torch.full((max(p, 1), 2), -7, dtype=torch.int64, device=DEV)
    weights = torch.full((max(p, 1),), -7.0, dtype=torch.float32, device=DEV)
    count = ctypes.c_int64(-7)
    with torch.cuda.device(dev.device):
        rc = lib.mde_edges_count_unique(n, p, _lib.ptr(dev) if p else None, _lib.ptr(edges), _lib.ptr(weights),
                                        ctypes.byref(count), _lib.stream_ptr(dev.device))
    m = count.value
    return rc, edges[:max(m, 0)].cpu().numpy(), weights[:max(m, 0)].cpu().numpy()


def test_count_unique_matches_the_restatement():
    """5000 rows over n = 97: multiplicities 1 .. 5 in both orientations, self pairs and rows with -1 (empty slots),
    shuffled; edges and float weights equal the numpy restatement exactly.  Then no rows, and only invalid rows."""
    rng = np.random.default_rng(7)
    n = 97
    base = np.array([ref.pair_of_index(n, int(i)) for i in rng.choice(ref.n_pairs(n), 1800, replace=False)])
    rows = np.repeat(base, rng.integers(1, 6, len(base)), axis=0)
    flip = rng.random(len(rows)) < 0.5
    rows[flip] = rows[flip][:, ::-1]
    selfs = np.repeat(rng.integers(0, n, 150), 2).reshape(-1, 2)
    empty = np.stack([rng.integers(0, n, 150), np.full(150, -1)], 1)
    empty[::3] = empty[::3][:, ::-1]
    empty[1::3] = -1
    rows = np.concatenate([rows, selfs, empty])
    assert len(rows) >= 5000
    rows = rng.permutation(rows)[:5000]
    want_e, want_w = ref.count_unique(rows)
    assert want_w.max() == 5.0 and want_w.min() == 1.0 and (rows == -1).any() and (rows[:, 0] == rows[:, 1]).any()
    rc, e, w = _count_unique(n, rows)
    assert rc == 0
    np.testing.assert_array_equal(e, want_e)
    np.testing.assert_array_equal(w, want_w.astype(np.float32))
    rc, e, w = _count_unique(n, np.zeros((0, 2), dtype=np.int64))
    assert rc == 0 and len(e) == 0 and len(w) == 0
    rc, e, w = _count_unique(n, [[4, 4], [-1, 3], [3, -1], [-1, -1], [96, 96]])
    assert rc == 0 and len(e) == 0 and len(w) == 0


# ---------------------------------------------------------------- items outside [0, n_items)
# (n_items, rows, index of the first bad row): an item equal to n, a negative one, and the pair that used to come
# back as another edge (n = 10: (0, 15) has the key of (1, 5))
BAD_LISTS = {
    "index-n": (30, [[0, 1], [2, 3], [4, 5], [29, 30], [7, 8], [30, 2]], 3),
    "negative": (30, [[0, 1], [2, 3], [-1, 5], [7, 8]], 2),
    "aliases-another-edge": (10, [[0, 15], [2, 3]], 0),
}


def _dedup(n, rows):
    from pymde_amd import preprocess
    return preprocess.deduplicate_edges(torch.tensor(rows), n_items=n)


def _sample(n, rows):
    from pymde_amd import preprocess
    return preprocess.sample_edges(n, 5, exclude=torch.tensor(rows), seed=0)


def _dissimilar(n, rows):
    from pymde_amd import preprocess
    return preprocess.dissimilar_edges(n, torch.tensor(rows), seed=0)


def _from_edges(n, rows):
    import pymde_amd
    return pymde_amd.Graph.from_edges(torch.tensor(rows), n_items=n)


@pytest.mark.parametrize("case", sorted(BAD_LISTS))
@pytest.mark.parametrize("door", [_dedup, _sample, _dissimilar, _from_edges],
                         ids=["deduplicate_edges", "sample_edges", "dissimilar_edges", "Graph.from_edges"])
def test_items_outside_the_range_are_refused(door, case):
    n, rows, first = BAD_LISTS[case]
    with pytest.raises(ValueError, match=rf"row {first} "):
        door(n, rows)
    good = [r for r in rows if 0 <= min(r) and max(r) < n]
    door(n, good)                                      # the rest of the list is fine


@pytest.mark.parametrize("case", sorted(BAD_LISTS))
def test_count_unique_refuses_items_outside_the_range(case):
    from pymde_amd import _lib
    n, rows, first = BAD_LISTS[case]
    rows = [[-2 if x == -1 else x for x in r] for r in rows]      # -1 stays the documented empty slot
    rc, _, _ = _count_unique(n, rows)
    assert rc == _lib.MDE_E_INVALID
    assert f"row {first} " in _lib.last_error()
    rc, e, w = _count_unique(n, [[-1 if x == -2 else x for x in r] for r in rows if max(r) < n])
    assert rc == 0 and len(e) == len(w) > 0
