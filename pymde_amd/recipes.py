"""Recipes that build MDE problems from data (the callers either side of the hot path).

``preserve_distances`` for data matrices [ref: pymde/recipes.py:103-218,
pymde/preprocess/data_matrix.py:11-88] is built from the GPU pieces of this package: the edge
sampler (``preprocess.sample_edges``, row f1) and the edge-order distance kernel with
``d = n_features`` (``mde_distances``, row f4); graph inputs use the batched shortest-path kernel (``graph.shortest_paths``,
row f3).  ``preserve_neighbors`` [ref: recipes.py:221-448] adds the exact GPU k-NN graph
(``preprocess.k_nearest_neighbors`` for data matrices, row f2; ``graph.k_nearest_neighbors`` under the
shortest-path metric for graphs, row f3) and the spectral initialiser; ``laplacian_embedding``
[ref: recipes.py:451-503] is the quadratic, standardized special case.
"""
import torch

from pymde_amd import _lib
from pymde_amd import affinity as _affinity
from pymde_amd import binary as _binary
from pymde_amd import constraints
from pymde_amd import dense as _dense
from pymde_amd import graph as _graph
from pymde_amd import landmarks as _landmarks
from pymde_amd import metrics as _metrics
from pymde_amd import ordinal as _ordinal
from pymde_amd import preprocess
from pymde_amd import problem
from pymde_amd import quality
from pymde_amd import util
from pymde_amd import quadratic
from pymde_amd import sparse as _sparse
from pymde_amd.functions import losses, penalties
from pymde_amd.pca import check_arguments as _pca_check_arguments


class EdgeGraph(object):
    """Edges with one value per edge (the role ``pymde.Graph`` plays for recipe outputs)."""

    def __init__(self, edges, values, n_items):
        self.edges = edges
        self.distances = values
        self.weights = values
        self.n_items = int(n_items)


def distances(data, retain_fraction=1.0, seed=None, device=None, metric="euclidean"):
    """Distances (Euclidean by default) between (a sample of) the pairs of rows of a data matrix
    [ref: preprocess/data_matrix.py:11-88].  All ``n (n-1)/2`` pairs when ``retain_fraction >= 1``,
    otherwise a uniform sample of that fraction.

    ``data`` is a dense ``np.ndarray`` / ``torch.Tensor`` or a sparse data matrix (scipy sparse, any
    format, or a torch sparse COO / CSR tensor); sparse distances are summed over the union of the
    two rows' columns (``mde_sparse_distances``), so near-duplicate rows come out near zero.

    ``metric``: ``"euclidean"``, ``"cosine"``, ``"correlation"`` or ``"manhattan"`` (aliases ``"l2"``,
    ``"l1"``, ``"cityblock"``), as ``scipy.spatial.distance`` defines them; the distances returned are in
    the metric's own units.  Dense data: one pass over the two original rows per pair, sums in double
    (``mde_pair_distances_metric``), so near-duplicate rows keep their small cosine / correlation
    distances.  Sparse data: cosine scales the rows to unit length and halves the squared sparse distance;
    correlation and Manhattan densify (an error if the dense copy does not fit).  A row without a
    direction (all zero under cosine, constant under correlation) is an error.

    A ``BitMatrix`` (``pymde_amd.binary``) gives its own Jaccard or Hamming distances, with the bits the searches
    give each pair (``mde_bits_pair_distances``); ``metric`` stays at its default beside it."""
    if _binary.is_bits(data):
        _binary.check_metric(metric)
        if device is not None:
            data = data.to(util.require_cuda_device(device))
        edges = _distance_edges(data.shape[0], retain_fraction, seed, data.device)
        return EdgeGraph(edges, _binary.pair_distances(data, edges), data.shape[0])
    metric = _metrics.resolve(metric)
    if metric != _metrics.EUCLIDEAN:
        return _metric_distances(data, retain_fraction, seed, device, metric)
    if _sparse.is_sparse(data):
        csr = _sparse.to_device_csr(data, device)
        edges = _distance_edges(csr.n, retain_fraction, seed, csr.device)
        lib = _lib.load()
        delta = torch.empty(edges.shape[0], dtype=torch.float32, device=csr.device)
        with torch.cuda.device(csr.device):
            _lib.check(lib.mde_sparse_distances(csr.n, csr.n_features, csr.nnz, _lib.ptr(csr.indptr),
                                                _lib.ptr(csr.indices), _lib.ptr(csr.values), edges.shape[0],
                                                _lib.ptr(edges), _lib.ptr(delta), _lib.stream_ptr(csr.device)))
        return EdgeGraph(edges, delta, csr.n)
    if not isinstance(data, torch.Tensor):
        data = torch.as_tensor(data)
    if device is None:
        device = data.device if data.is_cuda else util.get_default_device()
    device = util.require_cuda_device(device)
    data = data.to(device=device, dtype=torch.float32).contiguous()
    n, nf = int(data.shape[0]), int(data.shape[1])
    edges = _distance_edges(n, retain_fraction, seed, device)
    lib = _lib.load()
    delta = torch.empty(edges.shape[0], dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.mde_distances(n, edges.shape[0], _lib.ptr(edges), _lib.ptr(data), nf,
                                     _lib.ptr(delta), _lib.stream_ptr(device)))
    return EdgeGraph(edges, delta, n)


def _metric_distances(data, retain_fraction, seed, device, metric):
    """``distances`` under a metric other than Euclidean."""
    if _sparse.is_sparse(data):
        csr = _sparse.to_device_csr(data, device)
        if metric == _metrics.COSINE:
            csr = _metrics.normalized_csr(csr)
            edges = _distance_edges(csr.n, retain_fraction, seed, csr.device)
            chord = torch.empty(edges.shape[0], dtype=torch.float32, device=csr.device)
            with torch.cuda.device(csr.device):
                _lib.check(_lib.load().mde_sparse_distances(
                    csr.n, csr.n_features, csr.nnz, _lib.ptr(csr.indptr), _lib.ptr(csr.indices),
                    _lib.ptr(csr.values), edges.shape[0], _lib.ptr(edges), _lib.ptr(chord),
                    _lib.stream_ptr(csr.device)))
            return EdgeGraph(edges, 0.5 * chord * chord, csr.n)      # |u - v|^2 = 2 (1 - cos) for unit rows
        if not preprocess._densify_sparse_knn(csr.n, csr.n_features, csr.nnz, csr.device):
            raise ValueError(
                f"metric='{metric}' densifies sparse data, and the dense copy of this {csr.n} x "
                f"{csr.n_features} matrix does not fit in the device memory allowed for it; "
                "metric='cosine' and 'euclidean' have a sparse kernel")
        data = csr.to_dense()
    else:
        if not isinstance(data, torch.Tensor):
            data = torch.as_tensor(data)
        if device is None:
            device = data.device if data.is_cuda else util.get_default_device()
        device = util.require_cuda_device(device)
        data = data.to(device=device, dtype=torch.float32).contiguous()
    _metrics.check_rows(data, metric)
    n = int(data.shape[0])
    edges = _distance_edges(n, retain_fraction, seed, data.device)
    return EdgeGraph(edges, _metrics.pair_distances(data, edges, metric), n)


def _distance_edges(n, retain_fraction, seed, device):
    """All pairs i < j when ``retain_fraction >= 1``, otherwise a uniform sample of that fraction."""
    all_edges = n * (n - 1) // 2
    max_distances = int(retain_fraction * all_edges)
    if max_distances <= 0:
        raise ValueError("max_distances must be positive")
    if max_distances >= all_edges:
        return util.all_edges(n).to(device).contiguous()
    return preprocess.sample_edges(n, max_distances, seed=seed, device=device)


def _remove_anchor_anchor_edges(edges, data, anchors):
    """Drop edges whose two endpoints are both anchors: they are pinned by the constraint
    [ref: recipes.py:15-100]."""
    anchors = torch.as_tensor(anchors).to(edges.device)
    if anchors.numel() == 0:
        return edges, data
    both = torch.isin(edges[:, 0], anchors) & torch.isin(edges[:, 1], anchors)
    return edges[~both].contiguous(), data[~both].contiguous()


def preserve_distances(data, embedding_dim=2, loss=losses.Absolute, constraint=None,
                       max_distances=5e7, device=None, verbose=False, seed=None, metric="euclidean", dense=False,
                       landmarks=None, weights=None, landmark_selection="uniform", init="random", ordinal=False):
    """An MDE problem that preserves the pairwise distances (Euclidean by default) of a data matrix
    (rows = items) [ref: recipes.py:103-218].  At most ``max_distances`` pairs are used, sampled
    uniformly; with ``Standardized()`` the distances are rescaled to the constraint's natural
    length.  ``data`` is a dense ``np.ndarray`` / ``torch.Tensor``, a sparse data matrix (scipy
    sparse or a torch sparse COO / CSR tensor -- a data matrix, not an adjacency matrix), or a
    ``Graph``.  ``metric`` (data matrices only) as for ``distances``: the deviations are in the metric's
    own units, and ``Standardized()`` rescales them as it does Euclidean ones.  Call ``.embed()`` on the
    result.

    ``dense=True`` returns a ``DenseMDE`` over EVERY pair instead: no edge list, the distances are formed on
    the fly in each evaluation (``pymde_amd.dense``).  ``max_distances`` and ``seed`` are not consulted: nothing
    is sampled.  Data matrices under ``"euclidean"``, ``"cosine"`` or ``"correlation"`` only: a ``Graph`` or
    ``metric="manhattan"`` is a ``ValueError``.  ``Standardized()`` rescales the deviations as above, with
    their rms over all pairs from one ``quality.pair_moments`` pass.  With ``Anchored`` no pair is removed:
    the anchor-anchor pairs add a constant to the value of the problem and nothing to the gradient of the free
    rows.

    ``landmarks=m`` (``2 <= m < n``; implies the dense path) returns a ``dense.LandmarkMDE``: landmark MDS.  ``m``
    rows, drawn uniformly without replacement from ``seed``, are embedded with a ``DenseMDE`` over all their pairs
    and every other row is placed against them with a ``DensePlacement`` -- O(m^2 + n m) pairs per sweep instead
    of O(n^2), which is how all-pairs distance preservation reaches a million rows.  ``constraint`` must be
    ``None`` or ``Centered()``: the placed rows are unconstrained, so ``Standardized`` and ``Anchored`` are a
    ``ValueError``.  ``max_distances`` is not consulted.  Score the result with
    ``quality.stress(data, X, sample=...)``.  ``landmark_selection`` (with ``landmarks=m`` only): ``"uniform"`` (the
    default, that draw), ``"farthest"`` or ``"kmeans++"``: the landmarks ``pymde_amd.landmarks.select`` chooses under
    ``metric`` and ``seed``, which cover the data where a uniform draw follows its density; the problem's
    ``landmark_radius`` is then their covering radius.

    ``weights=p`` (with ``dense=True`` or ``landmarks=m`` only): a real number ``p >= 0``; every pair is weighed by
    ``D^-p`` as ``DenseMDE(weights=p)`` does it (``loss=Quadratic, weights=1`` is Sammon mapping), in both stages of
    the landmark path.  A weight matrix is a ``ValueError`` here: build the ``DenseMDE`` directly.  The edge-list
    path takes its weights through the loss (``WeightedQuadratic``).

    ``init`` (with ``dense=True`` or ``landmarks=m`` only): ``"random"`` (the default) or ``"classical"``, the
    ``init`` of ``DenseMDE`` and ``LandmarkMDE``: ``embed()`` then starts from the classical scaling of the
    deviations (and, on the landmark path, from the triangulation of the other rows against the landmarks).

    ``ordinal=True`` (the edge-list path only) returns a ``pymde_amd.OrdinalMDE`` over the same edges and deviations:
    non-metric MDS, which uses the order of the deviations and not their values (``pymde_amd.ordinal``); ``loss``
    must then be unweighted.  With ``dense=True``, ``landmarks=`` or an ``Anchored`` constraint it is a
    ``ValueError``."""
    if ordinal and (dense or landmarks is not None or isinstance(constraint, constraints.Anchored)):
        raise ValueError("`ordinal=True` applies to the edge-list path without anchors: not with dense=True, "
                         "landmarks=m or an Anchored constraint")
    _dense.check_init(init)
    if init != "random" and landmarks is None and not dense:
        raise ValueError("`init` applies to the dense problems (dense=True or landmarks=m); the edge-list problem "
                         "starts where its constraint's initialization puts it (pass embed(X=...) for another start)")
    if weights is not None:
        _dense.parse_weights(weights, allow_matrix=False)
        if landmarks is None and not dense:
            raise ValueError("`weights` applies to the dense problems (dense=True or landmarks=m); the edge-list "
                             "problem is weighed through its loss, e.g. losses.WeightedQuadratic")
    landmark_selection = _landmarks.resolve_selection(landmark_selection)
    if landmarks is None and landmark_selection != _landmarks.UNIFORM:
        raise ValueError("`landmark_selection` chooses the rows of the landmark path; pass landmarks=m with it")
    if landmarks is not None:
        return _dense.LandmarkMDE(data, landmarks, embedding_dim=embedding_dim, loss=loss, constraint=constraint,
                                  metric=metric, seed=seed, device=device, weights=weights,
                                  selection=landmark_selection, init=init)
    if dense:
        return _preserve_distances_dense(data, embedding_dim, loss, constraint, device, verbose, metric, weights,
                                         init)
    metric = _metrics.resolve(metric)
    is_graph = isinstance(data, _graph.Graph)
    if is_graph:
        _metrics.check_graph(metric)
    if _binary.is_bits(data):
        _binary.check_metric(metric)
    if not is_graph and not isinstance(data, torch.Tensor) and not hasattr(data, "shape"):
        raise ValueError("`data` must be a np.ndarray/torch.Tensor/sparse data matrix, or a pymde_amd.Graph.")
    n_items = data.n_items if is_graph else int(data.shape[0])
    n_all_edges = n_items * (n_items - 1) / 2
    retain_fraction = max_distances / n_all_edges
    if verbose:
        problem.LOGGER.info(f"Computing {int(min(max_distances, n_all_edges))} distances")
    if is_graph:
        # original distance = length of the shortest path between the two nodes (row f3)
        graph = _graph.shortest_paths(data, retain_fraction=retain_fraction,
                                      seed=0 if seed is None else seed)
    else:
        graph = distances(data, retain_fraction=retain_fraction, seed=seed, device=device, metric=metric)
    edges, deviations = graph.edges, graph.distances
    if ordinal:
        return _ordinal.OrdinalMDE(n_items, embedding_dim, edges, deviations, loss=loss, constraint=constraint,
                                   device=edges.device)
    if constraint is None:
        constraint = constraints.Centered()
    elif isinstance(constraint, constraints._Standardized):
        deviations = preprocess.scale(deviations,
                                      constraint.natural_length(n_items, embedding_dim).to(deviations.device))
    elif isinstance(constraint, constraints.Anchored):
        edges, deviations = _remove_anchor_anchor_edges(edges, deviations, constraint.anchors)
    return problem.MDE(n_items=n_items, embedding_dim=embedding_dim, edges=edges,
                       distortion_function=loss(deviations), constraint=constraint,
                       device=edges.device)


def preserve_geodesics(data, embedding_dim=2, n_neighbors=15, landmarks=None, *, loss=losses.Quadratic,
                       landmark_selection="farthest", init=None, metric="euclidean", seed=None, device=None,
                       verbose=False, connect=False, **search):
    """Preserve the geodesic distances of the data: landmark MDS under the shortest-path metric of a neighbour graph
    (Landmark Isomap, de Silva and Tenenbaum); returns the ``dense.LandmarkMDE`` of ``LandmarkMDE.from_graph``.

    ``data``: a data matrix, whose ``preprocess.neighbor_graph(data, n_neighbors, metric=metric, **search)`` is used
    (``search``: the keywords of the k-NN search), or a ``Graph``, used as it is with its values as edge lengths.
    ``landmarks``: how many (``None``: ``min(1000, n // 2)``), chosen by ``landmark_selection`` (``"farthest"``, the
    default, or ``"uniform"``).  ``init``: ``"random"``, ``"classical"``, or ``None``: classical when every (node,
    landmark) pair is joined by a path, random otherwise (one logged line says why).  The cost is one shortest-path
    solve from the landmarks, O(n m) memory; a graph of several components is embedded with the pairs across
    components left out, unless ``connect=`` joins the components first.

    ``connect`` (data matrices only; default False: nothing changes): ``True`` or ``"pairs"`` joins every two
    connected components of the neighbour graph by their nearest pair of rows, ``"tree"`` by the minimum spanning
    tree of those pairs (``preprocess.connect_components``, kept on the returned problem as ``mde.connection``).  No
    pair is missing then, the components are placed relative to each other, and ``init=None`` resolves to
    ``"classical"``.  With a ``Graph`` as ``data`` it is a ``ValueError`` -- there are no rows to measure between the
    components; ``graph.connected_components`` is what such a caller can use."""
    _binary.refuse(data, "preserve_geodesics")
    if init is not None:
        _dense.check_init(init)
    rule = preprocess.resolve_connect(connect) if connect else None
    connection = None
    landmark_selection = _landmarks.resolve_selection(landmark_selection)
    if landmark_selection == _landmarks.KMEANSPP:
        raise ValueError("landmark_selection='kmeans++' has no graph form; the selections here are 'farthest' and "
                         "'uniform'")
    if isinstance(data, _graph.Graph):
        _metrics.check_graph(_metrics.resolve(metric))
        if rule is not None:
            raise ValueError("connect= measures between the rows of a data matrix, and a Graph has none; "
                             "graph.connected_components reports the components of a Graph")
        graph = data
    else:
        if not isinstance(data, torch.Tensor) and not hasattr(data, "shape"):
            raise ValueError("`data` must be a np.ndarray/torch.Tensor/sparse data matrix, or a pymde_amd.Graph.")
        n_items = int(data.shape[0])
        if landmarks is not None:
            _dense.check_landmarks(landmarks, n_items, None)
        if verbose:
            problem.LOGGER.info(f"Building the {n_neighbors}-nearest-neighbour graph of {n_items} rows")
        graph = preprocess.neighbor_graph(data, n_neighbors, metric=metric, device=device, verbose=verbose, **search)
        if rule is not None:
            connection = preprocess.connect_components(data, graph, bridges=rule, metric=metric, device=device)
            graph = connection.graph
            if verbose:
                problem.LOGGER.info(f"The neighbour graph has {connection.n_components} connected component(s); "
                                    f"joined by {int(connection.bridges.shape[0])} bridge(s) ('{rule}')")
    if landmarks is None:
        landmarks = min(1000, graph.n_items // 2)
    if verbose:
        problem.LOGGER.info(f"Shortest paths from {landmarks} landmarks ({landmark_selection}) to "
                            f"{graph.n_items} nodes")
    mde = _dense.LandmarkMDE._build_from_graph(graph, landmarks, embedding_dim, loss, None, seed,
                                               landmark_selection, init, None, None)
    if connection is not None:
        mde.connection = connection
    return mde


def _preserve_distances_dense(data, embedding_dim, loss, constraint, device, verbose, metric, weights=None,
                              init="random"):
    """``preserve_distances(dense=True)``: the ``DenseMDE`` over every pair of the rows of ``data``."""
    metric = _dense.check_source(data, metric)
    if not isinstance(data, torch.Tensor) and not hasattr(data, "shape"):
        raise ValueError("`data` must be a np.ndarray/torch.Tensor/sparse data matrix for a dense problem.")
    n_items = int(data.shape[0])
    _dense.loss_spec(loss)
    deviation_scale = 1.0
    if isinstance(constraint, constraints._Standardized):
        if device is None:
            device = data.device if isinstance(data, torch.Tensor) and data.is_cuda else util.get_default_device()
        device = util.require_cuda_device(device)
        if verbose:
            problem.LOGGER.info(f"Computing the rms of all {n_items * (n_items - 1) // 2} distances")
        # (the embedding side of the pass is not used: one column of zeros)
        moments = quality.pair_moments(data, torch.zeros((n_items, 1), device=device), metric=metric)
        rms = (moments.sum_dd / moments.count) ** 0.5
        deviation_scale = float(constraint.natural_length(n_items, embedding_dim)) / rms
    return _dense.DenseMDE(data, embedding_dim=embedding_dim, loss=loss, constraint=constraint, metric=metric,
                           deviation_scale=deviation_scale, device=device, weights=weights, init=init)


def preserve_neighbors(data, embedding_dim=2, attractive_penalty=penalties.Log1p,
                       repulsive_penalty=penalties.Log, constraint=None, n_neighbors=None,
                       repulsive_fraction=None, max_distance=None, init="quadratic", device=None,
                       verbose=False, seed=None, approximate_neighbors=False, metric="euclidean",
                       neighbor_precision="float32", n_components=None, weights=None):
    """An MDE problem that preserves the k-nearest-neighbour structure of a data matrix
    (rows = items) [ref: recipes.py:221-448]: k-NN graph (weights 1 / 2), optional spectral
    initialisation, uniformly sampled repulsive edges (weight -1), ``PushAndPull`` of the two
    penalties.  ``data`` is a dense ``np.ndarray`` / ``torch.Tensor``, a sparse data matrix (scipy
    sparse or a torch sparse COO / CSR tensor; a data matrix, not an adjacency matrix), or a
    ``Graph``: neighbourhoods are then taken under its shortest-path metric.  Every stage runs on the
    GPU (rows f2, f3, a10, f1 of SURVEY section 8).

    ``approximate_neighbors`` (data matrices only): ``True`` builds the k-NN graph by the approximate
    inverted-file search of ``preprocess.k_nearest_neighbors(approximate=True)`` with its defaults, a dict
    ``{"n_lists": .., "n_probe": .., "n_refine": ..}`` sets those knobs (``n_refine``: neighbour-of-neighbour
    passes over the lists, default 0); ``False`` (the default) keeps the exact search.
    Recall depends on the data; ``verbose=True`` logs an estimate.

    ``metric`` (data matrices only): the distance in the original data under which neighbours are taken,
    as for ``preprocess.k_nearest_neighbors`` -- ``"euclidean"``, ``"cosine"``, ``"correlation"`` or
    ``"manhattan"``; ``max_distance`` is in its units.  The embedding side does not change.

    ``neighbor_precision`` (data matrices only): ``"bfloat16"`` builds the k-NN graph by the bfloat16
    shortlist with float32 re-ranking of ``preprocess.k_nearest_neighbors(precision="bfloat16")``; not with
    Manhattan or ``approximate_neighbors``.

    ``n_components`` (data matrices under the Euclidean metric only; default None: nothing changes): the k-NN
    graph is built on the scores of ``preprocess.principal_components(data, n_components, seed=0 if seed is None
    else seed)`` instead of the data -- the usual first step on wide sparse data, whose search otherwise costs
    time proportional to the number of features.  The scores are a dense matrix, so the exact, the approximate
    and the bfloat16 search all serve them.  ``max_distance`` is then in the units of the reduced space
    (distances between rows of the scores, which are at most the distances between rows of the data).  The
    fitted ``PrincipalComponents`` is kept on the returned problem as ``mde.principal_components``.

    ``weights`` (default None: the 1 / 2 weights, nothing changes): ``"perplexity"``, ``"umap"`` or a dict
    ``{"kind": .., "perplexity": .., "symmetrize": ..}`` weighs the attractive edges by the distances of the
    neighbour lists instead (``pymde_amd.affinity``): every row's kernel is calibrated to the perplexity (default
    ``n_neighbors / 3``) or, for umap, to ``log2(k)``, and the two directions of an edge are combined by
    ``symmetrize`` (``"mean"`` or ``"union"``; default mean for perplexity, union for umap).  The edges are those
    of the default; their weights are the symmetrised affinities times the one factor that makes their sum equal
    the number of directed list entries that count -- the sum of the 1 / 2 weights -- so that attraction keeps its
    balance against the -1 repulsive edges.  The factor is taken before any ``Anchored`` edge removal.  The
    ``affinity.Calibration`` is kept on the returned problem as ``mde.neighbor_calibration``."""
    affinity_spec = _affinity.parse_weights(weights)
    if _binary.is_bits(data):
        # its own distance, one exact search: the argument errors, before any device is required
        preprocess._check_bits_search(metric, approximate_neighbors not in (None, False), neighbor_precision, None)
        if n_components is not None:
            raise ValueError("n_components applies to float data matrices; a BitMatrix has no principal components")
    metric = _metrics.resolve(metric)
    is_graph = isinstance(data, _graph.Graph)
    if n_components is not None:
        if is_graph:
            raise ValueError("n_components applies to data matrices; a Graph has no columns to reduce")
        if metric != _metrics.EUCLIDEAN:
            raise ValueError(f"n_components needs metric='euclidean' (got '{metric}'): principal components keep "
                             "Euclidean distances, not cosine, correlation or Manhattan ones")
        if not hasattr(data, "shape"):
            data = torch.as_tensor(data)
        _pca_check_arguments(data.shape, n_components, sparse=_sparse.is_sparse(data))
    neighbor_precision = preprocess._check_precision_arguments(
        neighbor_precision, None, 1, metric, approximate_neighbors not in (None, False), is_graph)
    if is_graph:
        _metrics.check_graph(metric)
    knn_options = _approximate_options(approximate_neighbors)
    _metrics.check_approximate(metric, bool(knn_options))
    if is_graph and knn_options:
        raise ValueError("approximate_neighbors applies to data matrices; a Graph has no approximate search")
    is_bits = _binary.is_bits(data)
    if not is_graph and not is_bits and not isinstance(data, torch.Tensor) and not _sparse.is_sparse(data):
        data = torch.as_tensor(data)
    if device is None:
        if is_graph:
            device = data.edges.device
        elif is_bits:
            device = data.device
        else:
            device = data.device if isinstance(data, torch.Tensor) and data.is_cuda else util.get_default_device()
    device = util.require_cuda_device(device)
    n = int(data.n_items) if is_graph else int(data.shape[0])
    if n_neighbors is None:
        # the reference's default (recipes.py:318-321): about 1 % of all pairs as edges, within [5, 15]
        n_choose_2 = n * (n - 1) / 2
        n_neighbors = int(max(min(15, n_choose_2 * 0.01 / n), 5))
    if n_neighbors > n:
        problem.LOGGER.warning(
            "Requested n_neighbors {0} > number of items {1}. Setting n_neighbors to {2}".format(
                n_neighbors, n, n - 1))
        n_neighbors = n - 1
    if constraint is None and repulsive_penalty is not None:
        constraint = constraints.Centered()
    elif constraint is None and repulsive_penalty is None:
        constraint = constraints.Standardized()
    if is_graph and max_distance is None:
        # the reference bounds neighbourhoods on graphs (recipes.py:335-339)
        max_distance = (3 * torch.quantile(data.distances.float().cpu(), 0.75)).item()
    if verbose:
        problem.LOGGER.info(f"Computing {n_neighbors}-nearest neighbors, with max_distance={max_distance}")
    calibration = None
    if is_graph and affinity_spec is not None:
        edges, weights, calibration = _neighbor_affinities(affinity_spec, data, n_neighbors, max_distance,
                                                           graph_distances=True)
    elif is_graph:
        edges, weights = _graph.k_nearest_neighbors(data, k=n_neighbors, graph_distances=True,
                                                          max_distance=max_distance, verbose=verbose)
    else:
        fitted = None
        if n_components is not None:
            if verbose:
                problem.LOGGER.info(f"Reducing the data to {n_components} principal components")
            fitted = preprocess.principal_components(data, n_components, seed=0 if seed is None else seed,
                                                     device=device)
            data = fitted.scores
        if knn_options:
            knn_options.setdefault("seed", 0 if seed is None else seed)
            knn_options["verbose"] = verbose
        if metric != _metrics.EUCLIDEAN:
            knn_options["metric"] = metric
        if neighbor_precision != preprocess.FLOAT32:
            knn_options["precision"] = neighbor_precision
            knn_options["verbose"] = verbose
        if affinity_spec is not None:
            edges, weights, calibration = _neighbor_affinities(affinity_spec, data, n_neighbors, max_distance,
                                                               device=device, **knn_options)
        else:
            edges, weights = preprocess.k_nearest_neighbors(data, k=n_neighbors, max_distance=max_distance,
                                                            device=device, **knn_options)
    if isinstance(constraint, constraints.Anchored):
        edges, weights = _remove_anchor_anchor_edges(edges, weights, constraint.anchors)
    if init == "quadratic":
        if verbose:
            problem.LOGGER.info(f"Computing {init} initialization.")
        X_init = quadratic.spectral(n, embedding_dim, edges, weights, max_iter=1000, device=device, cg=True)
        if not isinstance(constraint, (constraints._Centered, constraints._Standardized)):
            constraint.project_onto_constraint(X_init, inplace=True)
    elif init == "random":
        X_init = constraint.initialization(n, embedding_dim, device)
    else:
        raise ValueError(f"Unsupported value '{init}' for keyword argument `init`; "
                         "the supported values are 'quadratic' and 'random'.")
    if repulsive_penalty is not None:
        if repulsive_fraction is None:
            # the standardization constraint already spreads the points: use a lower repulsion
            repulsive_fraction = 0.5 if isinstance(constraint, constraints._Standardized) else 1
        n_choose_2 = n * (n - 1) // 2
        n_repulsive = min(int(repulsive_fraction * edges.shape[0]), n_choose_2 - edges.shape[0])
        negative_edges = preprocess.sample_edges(n, n_repulsive, exclude=edges, seed=seed, device=device)
        negative_weights = -torch.ones(negative_edges.shape[0], dtype=torch.float32, device=device)
        if isinstance(constraint, constraints.Anchored):
            negative_edges, negative_weights = _remove_anchor_anchor_edges(
                negative_edges, negative_weights, constraint.anchors)
        edges = torch.cat([edges, negative_edges])
        weights = torch.cat([weights, negative_weights])
        f = penalties.PushAndPull(weights, attractive_penalty=attractive_penalty,
                                  repulsive_penalty=repulsive_penalty)
    else:
        f = attractive_penalty(weights)
    mde = problem.MDE(n_items=n, embedding_dim=embedding_dim, edges=edges, distortion_function=f,
                      constraint=constraint, device=device)
    mde._X_init = X_init
    if n_components is not None:
        mde.principal_components = fitted
    if calibration is not None:
        mde.neighbor_calibration = calibration
    # overlapping points make the average distortion non-differentiable: perturb them apart
    if bool((mde.distances(mde._X_init) == 0).any()):
        mde._X_init = mde._X_init + 1e-4 * torch.randn(mde._X_init.shape, device=device,
                                                       dtype=mde._X_init.dtype)
    return mde


def _neighbor_affinities(spec, data, k, max_distance, **search):
    """``(edges, weights, calibration)`` of ``affinity.neighbor_affinities`` for a parsed ``weights=`` value, the
    weights times the factor that makes their float64 sum the number of list entries that count."""
    kind, perplexity, rule = spec
    found = _affinity.neighbor_affinities(data, k, kind, perplexity=perplexity, symmetrize=rule,
                                          max_distance=max_distance, **search)
    n_entries = int((found.calibration.idx >= 0).sum())
    total = float(found.weights.double().sum())
    if not total > 0.0:
        raise ValueError("weights: the affinities of the neighbour lists sum to zero (no neighbour within "
                         "max_distance?)")
    weights = (found.weights.double() * (n_entries / total)).to(torch.float32)
    return found.edges, weights, found.calibration


def _sample_new_item_edges(n_old, n_new, count, exclude, generator, device):
    """Up to ``count`` distinct edges (i < j, sorted by (i, j)), each pairing a uniformly drawn new item
    (index >= n_old) with a uniformly drawn other item, old or new; none of them in ``exclude`` [p, 2]
    (i < j).  Drawn directly among the pairs that touch a new item, by rejection of the rare repeats."""
    n = n_old + n_new
    available = n_new * n_old + n_new * (n_new - 1) // 2 - int(exclude.shape[0])
    count = min(int(count), available)
    if count <= 0:
        return torch.empty((0, 2), dtype=torch.int64, device=device)
    exclude_keys = exclude[:, 0] * n + exclude[:, 1]
    found = torch.empty((0, 2), dtype=torch.int64, device=device)
    for _ in range(64):
        missing = count - int(found.shape[0])
        if missing <= 0:
            break
        draws = 2 * missing + 1024
        i = torch.randint(n_old, n, (draws,), generator=generator, device=device)
        j = torch.randint(0, n - 1, (draws,), generator=generator, device=device)
        j = j + (j >= i).to(torch.int64)                           # uniform over the items other than i
        lo, hi = torch.minimum(i, j), torch.maximum(i, j)
        keep = ~torch.isin(lo * n + hi, exclude_keys)
        found = preprocess.deduplicate_edges(torch.cat([found, torch.stack([lo[keep], hi[keep]], 1)]), n_items=n)
    if found.shape[0] > count:
        # the distinct draws are exchangeable: a uniform subset of them, kept in sorted order
        pick = torch.randperm(found.shape[0], generator=generator, device=device)[:count]
        found = found[torch.sort(pick).values]
    return found.contiguous()


def extend_embedding(data, X, new_data, attractive_penalty=penalties.Log1p, repulsive_penalty=penalties.Log,
                     n_neighbors=None, repulsive_fraction=None, max_distance=None, metric="euclidean",
                     device=None, verbose=False, seed=None, neighbor_precision="float32"):
    """An MDE problem that places new points into an existing embedding: ``data`` [n_old, n_features] are
    the rows already embedded, ``X`` [n_old, m] their embedding (the embedding dimension is taken from it;
    it is used as float32), ``new_data`` [n_new, n_features] the rows to add.  The reference documents
    this as an ``Anchored`` problem over old and new items and leaves the neighbour search to the user;
    here the search is ``preprocess.cross_nearest_neighbors`` (every stage on the GPU).

    The result is an ``MDE`` over ``n_old + n_new`` items, old items first, constrained by
    ``Anchored(anchors=arange(n_old), values=X)``: after ``.embed()`` the rows ``[:n_old]`` of the embedding
    equal ``X`` bit for bit and the rows ``[n_old:]`` are the new points.

    Attractive edges (weight 1): one edge between new item ``n_old + q`` and each of the ``n_neighbors``
    rows of ``data`` nearest to ``new_data[q]`` under ``metric`` (``"euclidean"``, ``"cosine"`` or
    ``"correlation"``; not Manhattan) and within ``max_distance`` (in the metric's units).  New points take
    their neighbours among the old rows only -- never among each other -- and the search is exact (there is
    no approximate cross search).  ``n_neighbors`` defaults as in ``preserve_neighbors``, computed from
    ``n_old``.  A new point with no neighbour within ``max_distance`` is an error: it would have repulsion
    only.  Repulsive edges (weight -1; none when ``repulsive_penalty`` is None):
    ``int(repulsive_fraction * n_attractive)`` of them (fraction 1 by default), each pairing a uniformly
    drawn new item with a uniformly drawn other item, old or new, with no self pair, no attractive pair and
    no repeat; the same ``seed`` gives the same edges.  Edges are stored with the smaller index first.

    The solve starts from ``X`` for the old rows and, for each new row, from the mean of its neighbours'
    rows of ``X`` (perturbed by 1e-4 when that leaves an edge of length zero).  An embedding that was
    ``Standardized`` does not stay standardized once new rows are added.

    ``neighbor_precision="bfloat16"`` takes the neighbours by
    ``preprocess.cross_nearest_neighbors(precision="bfloat16")``.

    Data that were reduced by principal components are extended in the reduced space, old and new rows in one
    coordinate system: with ``pc`` the fitted ``PrincipalComponents`` (``mde.principal_components``, or the
    result of ``preprocess.principal_components(data, 50)``),
        ``extend_embedding(pc.scores, X, pc.transform(new_data))``."""
    if _binary.is_bits(data) or _binary.is_bits(new_data):
        # two BitMatrix of one distance and width: the argument errors, before any device is required
        preprocess._check_bits_search(metric, False, neighbor_precision, None)
        _binary.check_pair(new_data, data)
    metric = _metrics.resolve(metric)
    neighbor_precision = preprocess.resolve_precision(neighbor_precision)
    if metric == _metrics.MANHATTAN:
        raise ValueError("extend_embedding has no Manhattan neighbour search; the metrics it serves are "
                         "'euclidean', 'cosine' and 'correlation'")
    for name, m in (("data", data), ("new_data", new_data)):
        if isinstance(m, _graph.Graph) or not hasattr(m, "shape") or len(m.shape) != 2:
            raise ValueError(f"`{name}` must be a data matrix (np.ndarray / torch.Tensor / sparse matrix)")
    if not isinstance(X, torch.Tensor):
        X = torch.as_tensor(X)
    n_old, n_new = int(data.shape[0]), int(new_data.shape[0])
    if X.dim() != 2 or int(X.shape[0]) != n_old:
        raise ValueError(f"`X` must hold one embedding vector per row of `data` ({n_old}); got shape "
                         f"{tuple(X.shape)}")
    if n_new < 1:
        raise ValueError("`new_data` needs at least one row")
    if device is None:
        on_gpu = [t.device for t in (X, data, new_data) if isinstance(t, torch.Tensor) and t.is_cuda]
        if _binary.is_bits(data):
            on_gpu.insert(0, data.device)
        device = on_gpu[0] if on_gpu else util.get_default_device()
    device = util.require_cuda_device(device)
    X = X.detach().to(device=device, dtype=torch.float32).contiguous()
    n, m = n_old + n_new, int(X.shape[1])
    if n_neighbors is None:
        n_neighbors = int(max(min(15, (n_old * (n_old - 1) / 2) * 0.01 / n_old), 5))
    if n_neighbors > n_old:
        problem.LOGGER.warning(f"Requested n_neighbors {n_neighbors} > number of embedded items {n_old}. "
                               f"Setting n_neighbors to {n_old}")
        n_neighbors = n_old
    if verbose:
        problem.LOGGER.info(f"Computing the {n_neighbors} nearest embedded rows of {n_new} new rows among "
                            f"{n_old}, with max_distance={max_distance}")
    idx, _ = preprocess.cross_nearest_neighbors(new_data, data, n_neighbors, max_distance=max_distance,
                                                metric=metric, device=device, precision=neighbor_precision)
    listed = idx >= 0
    n_alone = int((~listed.any(1)).sum())
    if n_alone:
        raise ValueError(f"{n_alone} of the {n_new} new points have no neighbour within max_distance="
                         f"{max_distance}: they would have repulsive edges only")
    new_items = torch.arange(n_old, n, device=device).unsqueeze(1).expand_as(idx)
    edges = torch.stack([idx[listed], new_items[listed]], 1)       # (old, new): the smaller index first
    weights = torch.ones(edges.shape[0], dtype=torch.float32, device=device)
    generator = torch.Generator(device=device)
    generator.manual_seed(int(util.np_rng().integers(0, 2 ** 63 - 1)) if seed is None else int(seed))
    if repulsive_penalty is not None:
        if repulsive_fraction is None:
            repulsive_fraction = 1
        n_repulsive = int(repulsive_fraction * edges.shape[0])
        if verbose:
            problem.LOGGER.info(f"Sampling {n_repulsive} repulsive edges at the new items")
        negative_edges = _sample_new_item_edges(n_old, n_new, n_repulsive, edges, generator, device)
        edges = torch.cat([edges, negative_edges])
        weights = torch.cat([weights, -torch.ones(negative_edges.shape[0], dtype=torch.float32, device=device)])
        f = penalties.PushAndPull(weights, attractive_penalty=attractive_penalty,
                                  repulsive_penalty=repulsive_penalty)
    else:
        f = attractive_penalty(weights)
    constraint = constraints.Anchored(anchors=torch.arange(n_old, device=device), values=X)
    mde = problem.MDE(n_items=n, embedding_dim=m, edges=edges, distortion_function=f, constraint=constraint,
                      device=device)
    if verbose:
        problem.LOGGER.info("Starting the new rows at the mean of their neighbours' embedding vectors")
    neighbours = X[idx.clamp(min=0)] * listed.unsqueeze(2)                       # [n_new, k, m]
    X_new = neighbours.sum(1) / listed.sum(1, keepdim=True)
    # overlapping points make the average distortion non-differentiable: perturb the new rows apart
    if bool((mde.distances(torch.cat([X, X_new])) == 0).any()):
        X_new = X_new + 1e-4 * torch.randn(X_new.shape, generator=generator, device=device, dtype=X_new.dtype)
    mde._X_init = torch.cat([X, X_new]).contiguous()
    return mde


def _approximate_options(approximate_neighbors):
    """Keywords of ``preprocess.k_nearest_neighbors`` for a recipe's ``approximate_neighbors`` value:
    False -> {} (the exact search), True -> approximate with the defaults, a dict -> approximate with
    its ``n_lists`` / ``n_probe`` / ``n_refine``."""
    if approximate_neighbors is None or approximate_neighbors is False:
        return {}
    if approximate_neighbors is True:
        return {"approximate": True}
    if isinstance(approximate_neighbors, dict):
        unknown = set(approximate_neighbors) - {"n_lists", "n_probe", "n_refine"}
        if unknown:
            raise ValueError(f"approximate_neighbors: unknown keys {sorted(unknown)}; "
                             "the knobs are 'n_lists', 'n_probe' and 'n_refine'")
        return dict(approximate_neighbors, approximate=True)
    raise ValueError("approximate_neighbors must be True, False or a dict {'n_lists': .., 'n_probe': ..}")


def laplacian_embedding(data, embedding_dim=2, n_neighbors=None, max_distance=None, init="quadratic",
                        device=None, verbose=False, approximate_neighbors=False, metric="euclidean",
                        neighbor_precision="float32", n_components=None, weights=None):
    """An MDE problem whose solution is a Laplacian embedding [ref: recipes.py:451-503]: the k-NN
    graph of ``preserve_neighbors`` with quadratic penalties, no repulsion and the standardization
    constraint.  ``data``, ``approximate_neighbors``, ``metric``, ``neighbor_precision`` and ``n_components``
    (the k-NN graph on that many principal components, seed 0; ``max_distance`` then in the reduced space's
    units) and ``weights`` (perplexity or UMAP affinities in place of the 1 / 2 weights) as for
    ``preserve_neighbors``."""
    return preserve_neighbors(data, embedding_dim=embedding_dim, attractive_penalty=penalties.Quadratic,
                              repulsive_penalty=None, n_neighbors=n_neighbors, max_distance=max_distance,
                              init=init, device=device, verbose=verbose,
                              approximate_neighbors=approximate_neighbors, metric=metric,
                              neighbor_precision=neighbor_precision, n_components=n_components, weights=weights)
