"""pymde_amd.affinity on the GPU (csrc/mde_affinity.hip) against the float64 replay of tests/_affinity_reference.py:
the two row calibrations, the symmetrisation bit for bit, determinism, every neighbour search as a source, and the
``weights=`` keyword of the recipes."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _affinity_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

N_VALUES = (1, 7, 257, 1000)
K_VALUES = (1, 2, 3, 15, 33, 64)
TRANSFORMS = ((True, 1.0), (False, 0.5), (False, 1.0))      # Euclidean d2, squared chord, the distance itself
KINDS = ("perplexity", "umap")


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV).contiguous()


def _lists(n, k, root, scale, seed):
    """Sorted random float32 lists whose distances sit at the scales 1e-3, 1 and 1e3 (one per row), with rows
    tied at the minimum, all-zero rows and rows with empty slots.  Row i lists i + 1, i + 2, ... (mod n)."""
    rng = np.random.default_rng(seed)
    idx = np.full((n, k), -1, np.int32)
    for c in range(min(k, n - 1)):
        idx[:, c] = (np.arange(n) + 1 + c) % n
    row_scale = rng.choice([1e-3, 1.0, 1e3], size=n)
    d = np.sort(rng.random((n, k)), 1) * row_scale[:, None]
    for i in range(n):
        if i % 5 == 1 and k > 2:
            d[i, :rng.integers(2, k + 1)] = d[i, 0]          # ties at the minimum (up to the whole row)
        if i % 7 == 3:
            d[i] = 0.0                                       # an all-zero row
        if i % 4 == 2:
            idx[i, rng.random(k) < 0.4] = -1                 # empty slots anywhere in the row
    val = ((d * d) if root else d) / (scale if not root else scale * scale)
    return idx, val.astype(np.float32), row_scale


@functools.lru_cache(maxsize=None)
def _case(ni, ki):
    """One shape: its lists, the GPU calibrations of both kinds and their float64 references, computed once."""
    from pymde_amd import affinity
    n, k = N_VALUES[ni], K_VALUES[ki]
    case = {"n": n, "k": k, "kinds": {}}
    for kind_i, kind in enumerate(KINDS):
        root, scale = TRANSFORMS[(ni + ki + kind_i) % 3]
        idx, val, row_scale = _lists(n, k, root, scale, seed=100 * ni + 10 * ki + kind_i)
        # every other shape cuts by max_value: the scale-1 rows lose their tails, the scale-1e3 rows everything
        max_value = None
        if (ni + ki) % 2 == 0:
            max_value = (0.7 / scale) ** 2 if root else 0.7 / scale          # distance 0.7 in the units of val
        perplexity = (None, 2.0, 5.0, k - 0.5)[(ni + ki) % 4] if kind == "perplexity" else None
        got = affinity.calibrate(_dev(idx), _dev(val), kind, perplexity=perplexity, root=root, scale=scale,
                                 max_value=max_value)
        want = ref.calibrate(idx, val, kind, perplexity, root, scale, max_value)
        case["kinds"][kind] = {
            "idx": idx, "val": val, "root": root, "scale": scale, "max_value": max_value,
            "perplexity": k / 3.0 if perplexity is None else perplexity,
            "got": tuple(t.cpu().numpy() for t in got), "want": want}
    return case


SHAPES = [(ni, ki) for ni in range(len(N_VALUES)) for ki in range(len(K_VALUES))]
SHAPE_IDS = ["n%d-k%d" % (N_VALUES[ni], K_VALUES[ki]) for ni, ki in SHAPES]


def _relative(got, want):
    """max |got - want| / |want| over finite non-zero ``want``; entries where ``want`` is 0 or inf must be equal."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    special = (want == 0) | np.isinf(want)
    assert np.array_equal(got[special], want[special])
    if special.all():
        return 0.0
    return float((np.abs(got[~special] - want[~special]) / np.abs(want[~special])).max())


@pytest.mark.parametrize("ni,ki", SHAPES, ids=SHAPE_IDS)
def test_calibration_matches_the_float64_reference(ni, ki):
    """|p - p_ref| <= 1e-6 p_ref + 1e-12 (the double bisection leaves ~87 * 2^-48 in any p float32 can hold, the
    rounding to float32 6e-8: a 16-fold margin), bandwidth and offset to 1e-6 relative with 0 and inf exact, the
    limit cases exactly, idx_out = idx with -1 at every cut entry.

    Largest deviations seen on an MI355X over all 24 shapes and both kinds: |p - p_ref| = 0.0594 of that bound
    (5.9e-8 p_ref, the float32 rounding; 2.98e-8 absolute); bandwidth and offset equal the reference rounded to
    float32, bit for bit."""
    case = _case(ni, ki)
    for kind in KINDS:
        c = case["kinds"][kind]
        idx_out, p, bandwidth, offset = c["got"]
        idx_ref, p_ref, bw_ref, off_ref, _ = c["want"]
        assert idx_out.dtype == np.int32 and p.dtype == np.float32
        assert np.array_equal(idx_out, idx_ref)
        cut = c["idx"] < 0
        if c["max_value"] is not None:
            cut = cut | ~(c["val"] <= np.float32(c["max_value"]))
        assert np.array_equal(idx_out, np.where(cut, -1, c["idx"]))
        err = np.abs(p.astype(np.float64) - p_ref)
        worst = float((err / (1e-6 * p_ref + 1e-12)).max())
        bw_err, off_err = _relative(bandwidth, bw_ref.astype(np.float32)), _relative(offset, off_ref.astype(np.float32))
        print(f"{kind} n={case['n']} k={case['k']}: max |p - p_ref| / (1e-6 p_ref + 1e-12) = {worst:.3g}, "
              f"max |p - p_ref| = {err.max():.3g}, bandwidth {bw_err:.3g}, offset {off_err:.3g}")
        assert worst <= 1.0, (kind, worst)
        assert bw_err <= 1e-6 and off_err <= 1e-6, (kind, bw_err, off_err)
        # the limit cases, exactly
        kept = idx_ref >= 0
        k_i = kept.sum(1)
        empty = k_i == 0
        assert (p[empty] == 0).all() and (bandwidth[empty] == 0).all() and (offset[empty] == 0).all()
        assert (p[~kept] == 0).all()
        if kind == "perplexity":
            exact = (bw_ref == 0) | np.isinf(bw_ref)
        else:
            g_zero = np.zeros(kept.shape, bool)
            for i in range(case["n"]):
                cols = np.flatnonzero(kept[i])
                g_zero[i, cols[ref.umap_gaps(ref.distances(c["val"][i][cols], c["root"], c["scale"]))[0] == 0]] = True
            assert (p[g_zero] == 1).all()                     # the nearest neighbour (and its ties) at full strength
            exact = g_zero.sum(1) == k_i                      # ... and the rows that are nothing else: all ones
        assert np.array_equal(p[exact], p_ref[exact].astype(np.float32))


@pytest.mark.parametrize("ni,ki", SHAPES, ids=SHAPE_IDS)
def test_rows_have_the_perplexity_and_the_membership_sum_asked_for(ni, ki):
    """Where the root exists, exp(H(p_i)) is within 1e-5 relative of the perplexity and the umap memberships sum
    to log2(k_i) within 1e-5 relative (k <= 64 float32 roundings of 6e-8 each), from the float32 output alone."""
    case = _case(ni, ki)
    c = case["kinds"]["perplexity"]
    p = c["got"][1].astype(np.float64)
    rows = np.flatnonzero(c["want"][4])
    for i in rows:
        q = p[i][p[i] > 0]
        assert abs(np.exp(-(q * np.log(q)).sum()) / c["perplexity"] - 1) <= 1e-5, i
    c = case["kinds"]["umap"]
    p = c["got"][1].astype(np.float64)
    solved = np.flatnonzero(c["want"][4])                     # (the floor did not replace the root)
    for i in solved:
        assert abs(p[i].sum() / np.log2((c["want"][0][i] >= 0).sum()) - 1) <= 1e-5, i
    if case["n"] >= 257 and case["k"] >= 15:                  # (k = 3 at perplexity k / 3 = 1 has limit cases only)
        assert len(rows) > 10 and len(solved) > 10


@functools.lru_cache(maxsize=None)
def _blob_lists(with_bound):
    """Euclidean lists of 500 x 8 data at k = 10 with an outlier row nobody lists; under the bound (the median
    10th-neighbour distance) the outlier keeps no entry either."""
    from pymde_amd import preprocess
    rng = np.random.default_rng(3)
    data = rng.standard_normal((500, 8)).astype(np.float32)
    data[17] += 40.0
    data = _dev(data)
    idx, d2, _, root, scale = preprocess._neighbor_lists(data, 10)
    assert root is True and scale == 1.0
    max_distance = float(d2[:, -1].sqrt().median()) if with_bound else None
    return data, idx, d2, max_distance


@pytest.mark.parametrize("with_bound", [False, True], ids=["all", "max_distance"])
@pytest.mark.parametrize("rule", ["mean", "union"])
def test_symmetrize_is_the_k_nn_graph_with_the_reference_weights_bit_for_bit(rule, with_bound):
    from pymde_amd import affinity, preprocess
    data, idx, d2, max_distance = _blob_lists(with_bound)
    bound = None if max_distance is None else max_distance ** 2
    cal = affinity.calibrate(idx, d2, "umap", root=True, max_value=bound)
    idx_out = cal.idx.cpu().numpy()
    assert not (idx_out == 17).any()                          # a row listed by nobody
    assert (idx_out[17] < 0).all() == with_bound              # ... and, under the bound, with no kept entry
    rng = np.random.default_rng(4)
    p = rng.random(idx_out.shape).astype(np.float32) * rng.choice(np.float32([1e-30, 1e-3, 1.0]), idx_out.shape)
    p[idx_out < 0] = 0
    edges, weights = affinity.symmetrize(cal.idx, _dev(p), rule)
    want_edges, ones_and_twos = preprocess.k_nearest_neighbors(data, 10, max_distance=max_distance)
    assert edges.dtype == torch.int64 and weights.dtype == torch.float32
    assert torch.equal(edges, want_edges)
    ref_edges, ref_weights = ref.symmetrize(idx_out, p, rule)
    assert np.array_equal(edges.cpu().numpy(), ref_edges)
    assert torch.equal(weights, _dev(ref_weights))
    # the 1 / 2 weights count the directions that the reference combined
    a_and_b = torch.as_tensor((ref.symmetrize(idx_out, (idx_out >= 0).astype(np.float32), "mean")[1] * 2), device=DEV)
    assert torch.equal(a_and_b, ones_and_twos)


def test_symmetrize_k1_and_an_underflowing_weight():
    from pymde_amd import affinity, preprocess
    data, _, _, _ = _blob_lists(False)
    idx, d2, _, _, _ = preprocess._neighbor_lists(data, 1)
    p = torch.full(idx.shape, 1e-30, device=DEV)
    for rule in ("mean", "union"):
        edges, weights = affinity.symmetrize(idx, torch.zeros_like(p), rule)
        assert torch.equal(edges, preprocess.k_nearest_neighbors(data, 1)[0])
        assert (weights == 0).all()                           # a zero weight, and the edges stay
        edges, weights = affinity.symmetrize(idx, p, rule)
        ref_edges, ref_weights = ref.symmetrize(idx.cpu().numpy(), p.cpu().numpy(), rule)
        assert np.array_equal(edges.cpu().numpy(), ref_edges) and torch.equal(weights, _dev(ref_weights))


@pytest.mark.parametrize("kind,rule", [("perplexity", "mean"), ("umap", "union")])
def test_same_bits_on_every_run_and_under_a_row_permutation(kind, rule):
    from pymde_amd import affinity
    _, idx, d2, max_distance = _blob_lists(True)
    n = idx.shape[0]

    def run(idx, d2):
        cal = affinity.calibrate(idx, d2, kind, root=True, max_value=max_distance ** 2)
        return cal, affinity.symmetrize(cal.idx, cal.conditionals, rule)
    cal, (edges, weights) = run(idx, d2)
    for _ in range(2):
        cal2, (edges2, weights2) = run(idx, d2)
        assert all(torch.equal(a, b) for a, b in zip(cal, cal2))
        assert torch.equal(edges, edges2) and torch.equal(weights, weights2)
    perm = torch.as_tensor(np.random.default_rng(5).permutation(n), device=DEV)      # row i moves to perm[i]
    inverse = torch.empty_like(perm)
    inverse[perm] = torch.arange(n, device=DEV)
    moved = torch.where(idx >= 0, perm[idx.long().clamp(min=0)].to(torch.int32), idx)
    cal3, (edges3, weights3) = run(moved[inverse].contiguous(), d2[inverse].contiguous())
    assert torch.equal(cal3.conditionals[perm], cal.conditionals)
    assert torch.equal(cal3.bandwidth[perm], cal.bandwidth) and torch.equal(cal3.offset[perm], cal.offset)
    back = inverse[edges3].sort(1).values
    order = torch.argsort(back[:, 0] * n + back[:, 1])
    assert torch.equal(back[order], edges) and torch.equal(weights3[order], weights)


def _cycle_with_chords():
    import pymde_amd
    n = 60
    ring = [(i, (i + 1) % n) for i in range(n)]
    chords = [(i, (i + 7) % n) for i in range(0, n, 5)]
    e = np.array(ring + chords, np.int64)
    lengths = np.where(np.arange(len(e)) < n, 1.0, 2.5).astype(np.float32)
    return pymde_amd.Graph.from_edges(_dev(e), _dev(lengths), n_items=n)


@pytest.mark.parametrize("source", ["cosine", "manhattan", "graph", "euclidean"])
def test_neighbor_affinities_is_calibrate_and_symmetrize_on_the_routes_own_lists(source):
    from pymde_amd import affinity, preprocess
    rng = np.random.default_rng(6)
    if source == "graph":
        data, k, options, transform, bound_d = _cycle_with_chords(), 6, {}, (False, 1.0), 2.0
    else:
        data, k = _dev(rng.standard_normal((300, 6)).astype(np.float32) + 0.5), 9
        options = {"metric": source}
        transform = {"cosine": (False, 0.5), "manhattan": (False, 1.0), "euclidean": (True, 1.0)}[source]
        bound_d = {"cosine": 0.25, "manhattan": 3.0, "euclidean": 1.6}[source]
    for kind, max_distance in (("perplexity", None), ("umap", bound_d)):
        found = affinity.neighbor_affinities(data, k, kind, max_distance=max_distance, **options)
        idx, values, bound, root, scale = preprocess._neighbor_lists(data, k, max_distance=max_distance, **options)
        assert (root, scale) == transform                     # cosine: the v / 2 of the squared chord
        cal = affinity.calibrate(idx, values, kind, root=root, scale=scale, max_value=bound)
        assert all(torch.equal(a, b) for a, b in zip(found.calibration, cal))
        edges, weights = affinity.symmetrize(cal.idx, cal.conditionals, "mean" if kind == "perplexity" else "union")
        assert torch.equal(found.edges, edges) and torch.equal(found.weights, weights)
        assert torch.equal(edges, preprocess.k_nearest_neighbors(data, k, max_distance=max_distance, **options)[0])
        want = ref.calibrate(idx.cpu().numpy(), values.cpu().numpy(), kind, None, root, scale, bound)
        assert np.array_equal(want[0], cal.idx.cpu().numpy())
        p = cal.conditionals.cpu().numpy().astype(np.float64)
        assert (np.abs(p - want[1]) <= 1e-6 * want[1] + 1e-12).all()
        # ... and the transform gives the metric's own distance: recomputed from the rows, bounded by max_distance
        d = ref.distances(values.cpu().numpy(), root, scale)
        kept = cal.idx.cpu().numpy() >= 0
        if max_distance is not None:
            assert (d[kept] <= max_distance * (1 + 1e-6)).all() and not kept.all() and kept.any()
        if source != "graph":
            x = data.cpu().numpy().astype(np.float64)
            a, b = x[:, None, :], x[idx.cpu().numpy().clip(min=0)]
            if source == "cosine":
                true = 1 - (a * b).sum(2) / (np.linalg.norm(a, axis=2) * np.linalg.norm(b, axis=2))
            else:
                true = np.abs(a - b).sum(2) if source == "manhattan" else np.linalg.norm(a - b, axis=2)
            assert np.allclose(d[kept], true[kept], rtol=1e-4, atol=1e-6)


def test_euclidean_affinities_match_the_reference_fed_the_distances():
    """The Euclidean route hands the kernel squared distances and root = True; the reference is fed sqrt(d2)."""
    from pymde_amd import affinity, preprocess
    data = _dev(np.random.default_rng(7).standard_normal((400, 5)).astype(np.float32))
    for kind in KINDS:
        found = affinity.neighbor_affinities(data, 15, kind)
        idx, d2, _, _, _ = preprocess._neighbor_lists(data, 15)
        d2 = d2.cpu().numpy()
        want = ref.calibrate(idx.cpu().numpy(), d2, kind, root=True)
        rows = [ref.perplexity_row(np.sqrt(r.astype(np.float64)), 5.0)[0] if kind == "perplexity"
                else ref.umap_row(np.sqrt(r.astype(np.float64)))[0] for r in d2[:50]]
        assert np.array_equal(np.stack(rows), want[1][:50])
        p = found.calibration.conditionals.cpu().numpy().astype(np.float64)
        assert (np.abs(p - want[1]) <= 1e-6 * want[1] + 1e-12).all()
        rule = "mean" if kind == "perplexity" else "union"
        ref_edges, ref_weights = ref.symmetrize(want[0], found.calibration.conditionals.cpu().numpy(), rule)
        assert np.array_equal(found.edges.cpu().numpy(), ref_edges)
        assert torch.equal(found.weights, _dev(ref_weights))


@functools.lru_cache(maxsize=None)
def _blobs():
    rng = np.random.default_rng(0)
    centres = 6.0 * rng.standard_normal((3, 10))
    data = centres[np.arange(600) % 3] + rng.standard_normal((600, 10))
    return _dev(data.astype(np.float32))


def _parts(mde):
    """(attractive edges, their weights, repulsive edges, their weights); an affinity that underflowed to 0 is an
    attractive edge still."""
    w = mde.distortion_function.weights
    return mde.edges[w >= 0], w[w >= 0], mde.edges[w < 0], w[w < 0]


def test_weights_none_is_the_default_bit_for_bit():
    import pymde_amd
    pymde_amd.seed(0)                                         # (the spectral start draws from torch's generator)
    a = pymde_amd.preserve_neighbors(_blobs(), n_neighbors=15, seed=0)
    pymde_amd.seed(0)
    b = pymde_amd.preserve_neighbors(_blobs(), n_neighbors=15, seed=0, weights=None)
    assert torch.equal(a.edges, b.edges)
    assert torch.equal(a.distortion_function.weights, b.distortion_function.weights)
    assert torch.equal(a._X_init, b._X_init)
    assert not hasattr(a, "neighbor_calibration") and not hasattr(b, "neighbor_calibration")


def test_weighted_recipes_keep_the_edges_and_the_balance_and_embed():
    """Neighbour overlap at k = 15 after embed(max_iter=40) on the 600 x 10 blobs, seed 0, on an MI355X: 0.269 with
    the 1 / 2 weights, 0.307 with weights="perplexity", 0.304 with weights="umap".  The 0.8 is a guard against
    collapse, not a claim that either weighting is better."""
    import pymde_amd
    from pymde_amd import quality
    data = _blobs()
    pymde_amd.seed(0)
    default = pymde_amd.preserve_neighbors(data, n_neighbors=15, seed=0)
    edges, ones_and_twos, negative_edges, _ = _parts(default)
    n_entries = float(ones_and_twos.double().sum())
    assert n_entries == 600 * 15
    overlap = {"default": float(quality.neighbor_overlap(data, default.embed(max_iter=40), 15))}
    for weights in ("perplexity", "umap", {"kind": "perplexity", "perplexity": 5, "symmetrize": "mean"}):
        pymde_amd.seed(0)
        mde = pymde_amd.preserve_neighbors(data, n_neighbors=15, seed=0, weights=weights)
        e, w, ne, nw = _parts(mde)
        assert torch.equal(e, edges)
        assert abs(float(w.double().sum()) / n_entries - 1) <= 1e-6
        assert torch.equal(ne, negative_edges) and (nw == -1).all()
        cal = mde.neighbor_calibration
        assert tuple(cal.idx.shape) == (600, 15) and int((cal.idx >= 0).sum()) == n_entries
        if isinstance(weights, dict):
            found = pymde_amd.affinity.neighbor_affinities(data, 15, "perplexity", perplexity=5, symmetrize="mean")
            assert torch.equal(found.calibration.conditionals, cal.conditionals)
            continue
        X = mde.embed(max_iter=40)
        assert bool(torch.isfinite(X).all())
        overlap[weights] = float(quality.neighbor_overlap(data, X, 15))
    print("neighbour overlap:", overlap)
    assert overlap["perplexity"] >= 0.8 * overlap["default"]
    assert overlap["umap"] >= 0.8 * overlap["default"]


def test_weighted_recipe_under_max_distance_and_anchors():
    """The factor counts the entries within max_distance, and is taken before the anchor-anchor edges go."""
    import pymde_amd
    from pymde_amd import preprocess
    data = _blobs()
    max_distance = float(preprocess._neighbor_lists(data, 15)[1].sqrt().median())
    plain = pymde_amd.preserve_neighbors(data, n_neighbors=15, seed=0, max_distance=max_distance, init="random")
    mde = pymde_amd.preserve_neighbors(data, n_neighbors=15, seed=0, max_distance=max_distance, init="random",
                                       weights="umap")
    e, w, _, _ = _parts(mde)
    pe, pw, _, _ = _parts(plain)
    assert torch.equal(e, pe) and 0 < float(pw.double().sum()) < 600 * 15
    assert abs(float(w.double().sum()) / float(pw.double().sum()) - 1) <= 1e-6
    anchors = torch.arange(100, device=DEV)
    anchored = pymde_amd.preserve_neighbors(
        data, n_neighbors=15, seed=0, max_distance=max_distance, init="random", weights="umap",
        constraint=pymde_amd.Anchored(anchors, torch.zeros((100, 2), device=DEV)))
    ae, aw, _, _ = _parts(anchored)
    both = (e < 100).all(1)
    assert torch.equal(ae, e[~both]) and torch.equal(aw, w[~both])


def test_laplacian_embedding_takes_the_weights():
    import pymde_amd
    mde = pymde_amd.laplacian_embedding(_blobs(), n_neighbors=15, weights="umap")
    plain = pymde_amd.laplacian_embedding(_blobs(), n_neighbors=15)
    assert torch.equal(mde.edges, plain.edges)
    w = mde.distortion_function.weights
    assert not torch.equal(w, plain.distortion_function.weights)
    assert abs(float(w.double().sum()) / (600 * 15) - 1) <= 1e-6
    assert mde.neighbor_calibration.bandwidth.shape == (600,)
    X = mde.embed(max_iter=40)
    assert X.shape == (600, 2) and bool(torch.isfinite(X).all())


def test_graph_recipe_takes_the_weights():
    import pymde_amd
    graph = _cycle_with_chords()
    plain = pymde_amd.preserve_neighbors(graph, n_neighbors=4, seed=0, init="random")
    mde = pymde_amd.preserve_neighbors(graph, n_neighbors=4, seed=0, init="random", weights="perplexity")
    e, w, _, _ = _parts(mde)
    pe, pw, _, _ = _parts(plain)
    assert torch.equal(e, pe) and abs(float(w.double().sum()) / float(pw.double().sum()) - 1) <= 1e-6


def test_bad_arguments_raise_value_errors():
    import pymde_amd
    from pymde_amd import affinity
    data = _blobs()
    idx = torch.zeros((4, 3), dtype=torch.int32, device=DEV)
    val = torch.ones((4, 3), device=DEV)
    with pytest.raises(ValueError, match="unknown affinity kind"):
        affinity.calibrate(idx, val, "heat")
    with pytest.raises(ValueError, match="unknown symmetrisation rule"):
        affinity.symmetrize(idx, val, "max")
    for bad in (0, -2.0):
        with pytest.raises(ValueError, match="perplexity must be"):
            affinity.calibrate(idx, val, perplexity=bad)
    with pytest.raises(ValueError, match="perplexity belongs to"):
        affinity.calibrate(idx, val, "umap", perplexity=5)
    with pytest.raises(ValueError, match="scale must be"):
        affinity.calibrate(idx, val, scale=0.0)
    with pytest.raises(ValueError, match="1 <= k <= 64"):
        affinity.calibrate(torch.zeros((4, 65), dtype=torch.int32, device=DEV), torch.ones((4, 65), device=DEV))
    with pytest.raises(ValueError, match="unknown keywords"):
        affinity.neighbor_affinities(data, 5, n_trees=3)
    with pytest.raises(ValueError, match="unknown affinity kind"):
        affinity.neighbor_affinities(data, 5, "heat")
    for bad, match in (("heat", "unknown affinity kind"), ({"kind": "umap", "perplexity": 5}, "perplexity belongs to"),
                       ({"kind": "perplexity", "perplexity": 0}, "perplexity must be"),
                       ({"symmetrize": "max"}, "unknown symmetrisation rule"), ({"sigma": 1}, "unknown keys"),
                       (2.0, "weights must be")):
        with pytest.raises(ValueError, match=match):
            pymde_amd.preserve_neighbors(data, weights=bad)
        with pytest.raises(ValueError, match=match):
            pymde_amd.laplacian_embedding(data, weights=bad)
