"""Approximate k-nearest-neighbour lists of a dense data matrix on the GPU: an inverted file (IVF) with
cluster-level probing (csrc/mde_ann.hip) [ref: preprocess/data_matrix.py:125-143 -- the reference turns to
pynndescent above 10 000 items].

  1. k-means on a sample of the rows splits them into ``n_lists`` lists (assignment by the
     query-against-base search with k = 1, centroids by a deterministic per-list sum);
  2. every row is assigned to its nearest centroid and the rows are sorted by list (stable: id order
     within a list);
  3. each list probes the ``n_probe`` lists whose centroids are nearest to its own, itself first;
  4. every query tile of 64 rows of a list is searched against the rows of its probed lists only;
  5. optionally (``n_refine``), neighbour-of-neighbour passes over the lists (``refine_lists``,
     csrc/mde_ann_refine.hip): every row is offered its reverse neighbours and the lists of its forward and
     reverse neighbours, which repairs the neighbours missed at the borders of the lists.

The host side here is plumbing (sampling, sorting, offsets, the tile list); every distance is computed
by the HIP kernels.  Recall depends on the data: it is high when the rows form clusters and poor on
structureless data such as an isotropic Gaussian, where neighbours straddle many lists.
``sampled_recall`` estimates it against the exact search.
"""
import heapq
import math

import torch

from pymde_amd import _lib

MIN_ITEMS = 10000        # below this the exact kernel runs (the reference's threshold)
MAX_K = 64
KMEANS_ITERS = 10
KMEANS_SAMPLE_PER_LIST = 128
TILE = 64
SELF, SCATTER = 1, 2     # mde_ann_search flags


def resolve_params(n, n_lists=None, n_probe=None):
    """(n_lists, n_probe) for n items: defaults round(sqrt(n)) and min(32, n_lists); n_lists is capped at n
    and n_probe at n_lists (every list probed).  Values below 1 raise ``ValueError``."""
    n = int(n)
    if n_lists is None:
        n_lists = max(1, int(round(math.sqrt(n))))
    if n_probe is None:
        n_probe = min(32, int(n_lists))
    n_lists, n_probe = int(n_lists), int(n_probe)
    if n_lists < 1:
        raise ValueError(f"n_lists must be at least 1 (got {n_lists})")
    if n_probe < 1:
        raise ValueError(f"n_probe must be at least 1 (got {n_probe})")
    n_lists = min(n_lists, n)
    n_probe = min(n_probe, n_lists)
    if MAX_K + 1 < n_probe < n_lists:
        raise ValueError(f"n_probe must be at most {MAX_K + 1}, or at least n_lists to probe every list "
                         f"(got n_probe={n_probe}, n_lists={n_lists})")
    return n_lists, n_probe


def tile_list(offsets, probe):
    """Query tiles (q_lo, q_hi, list) of every list, heaviest first, and their costs (host tensors).

    offsets: int64 [n_lists + 1] (host), probe: int64 [n_lists, n_probe] (host).  A tile's cost is the
    number of candidate rows it scans: the summed sizes of its list's probed lists."""
    sizes = offsets[1:] - offsets[:-1]
    n_tiles = (sizes + TILE - 1) // TILE
    lists = torch.repeat_interleave(torch.arange(sizes.shape[0], dtype=torch.int64), n_tiles)
    first = torch.cumsum(n_tiles, 0) - n_tiles
    j = torch.arange(lists.shape[0], dtype=torch.int64) - first[lists]
    lo = offsets[lists] + TILE * j
    hi = torch.minimum(lo + TILE, offsets[lists + 1])
    cost_list = sizes[probe].sum(1)
    cost = cost_list[lists]
    order = torch.sort(cost, descending=True, stable=True).indices
    tiles = torch.stack([lo, hi, lists], 1)[order].contiguous()
    return tiles, cost[order]


def imbalance(cost, slots):
    """Makespan of greedy list scheduling of the (heaviest first) tile costs on ``slots`` workgroup slots,
    over the ideal (total / slots): 1.0 is perfect balance."""
    cost = [int(c) for c in cost.tolist()]
    total = sum(cost)
    if total == 0:
        return 1.0
    slots = max(1, min(int(slots), len(cost)))
    heap = [0] * slots
    for c in cost:
        heapq.heapreplace(heap, heap[0] + c)
    return max(heap) / (total / slots)


def _row_sqnorm(X):
    lib = _lib.load()
    out = torch.empty(X.shape[0], dtype=torch.float32, device=X.device)
    _lib.check(lib.mde_row_sqnorm(X.shape[0], X.shape[1], _lib.ptr(X), _lib.ptr(out), _lib.stream_ptr(X.device)))
    return out


def search(Q, q_sqn, B, b_sqn, k, offsets, probe, tiles, q_map=None, b_map=None, n_qpos=None, n_bpos=None,
           flags=0):
    """Thin wrapper of ``mde_ann_search`` (device tensors; see include/mde_hip.h).  Returns (idx, d2)."""
    lib = _lib.load()
    n_q, nf = int(Q.shape[0]), int(Q.shape[1])
    n_b = int(B.shape[0])
    n_qpos = int(q_map.shape[0]) if q_map is not None else (n_q if n_qpos is None else int(n_qpos))
    n_bpos = int(b_map.shape[0]) if b_map is not None else (n_b if n_bpos is None else int(n_bpos))
    rows = n_q if flags & SCATTER else n_qpos
    idx = torch.empty((rows, k), dtype=torch.int32, device=Q.device)
    d2 = torch.empty((rows, k), dtype=torch.float32, device=Q.device)
    _lib.check(lib.mde_ann_search(nf, k, flags, n_q, _lib.ptr(Q), _lib.ptr(q_sqn), n_qpos, _lib.ptr(q_map),
                                  n_b, _lib.ptr(B), _lib.ptr(b_sqn), n_bpos, _lib.ptr(b_map),
                                  offsets.shape[0] - 1, _lib.ptr(offsets), probe.shape[1], _lib.ptr(probe),
                                  tiles.shape[0], _lib.ptr(tiles), _lib.ptr(idx), _lib.ptr(d2),
                                  _lib.stream_ptr(Q.device)))
    return idx, d2


def _whole(n_qpos, n_bpos, device):
    """offsets / probe / tiles of one list holding every base position, every query position probing it."""
    offsets = torch.tensor([0, n_bpos], dtype=torch.int64, device=device)
    probe = torch.zeros((1, 1), dtype=torch.int32, device=device)
    lo = torch.arange(0, n_qpos, TILE, dtype=torch.int64)
    tiles = torch.stack([lo, torch.clamp(lo + TILE, max=n_qpos), torch.zeros_like(lo)], 1)
    return offsets, probe, tiles.to(device)


def exact_search(Q, q_sqn, B, b_sqn, k, q_map=None, flags=0):
    """Exact k nearest rows of B for every query (rows of Q, or the rows q_map names), in query order."""
    n_qpos = int(q_map.shape[0]) if q_map is not None else int(Q.shape[0])
    offsets, probe, tiles = _whole(n_qpos, int(B.shape[0]), Q.device)
    return search(Q, q_sqn, B, b_sqn, k, offsets, probe, tiles, q_map=q_map, flags=flags)


def _sort_by_list(labels, n_lists):
    """Members sorted by list (stable: id order within a list) and the int64 offsets [n_lists + 1]."""
    order = torch.sort(labels, stable=True).indices
    counts = torch.bincount(labels, minlength=n_lists)
    offsets = torch.zeros(n_lists + 1, dtype=torch.int64, device=labels.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return order, offsets


def kmeans(X, sqn, n_lists, seed, iters=KMEANS_ITERS):
    """Centroids [n_lists, nf] of k-means on a seeded sample of the rows (initialised on sampled rows)."""
    n = int(X.shape[0])
    device = X.device
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    m = min(n, KMEANS_SAMPLE_PER_LIST * n_lists)
    sample = torch.randperm(n, generator=g, device=device)[:m].to(torch.int32)
    cent = X[sample[:n_lists].long()].contiguous()
    for _ in range(iters):
        labels = assign(X, sqn, cent, q_map=sample)
        order, offsets = _sort_by_list(labels, n_lists)
        update_centroids(X, sample[order].contiguous(), offsets, cent)
    return cent


def update_centroids(X, members, offsets, cent):
    """cent[l] = mean of the rows members[offsets[l]:offsets[l + 1]] of X, in place (``mde_ann_centroids``)."""
    lib = _lib.load()
    _lib.check(lib.mde_ann_centroids(X.shape[0], X.shape[1], _lib.ptr(X), members.shape[0], _lib.ptr(members),
                                     cent.shape[0], _lib.ptr(offsets), _lib.ptr(cent), _lib.stream_ptr(X.device)))


def assign(X, sqn, cent, q_map=None):
    """Nearest centroid of every row (or of the rows q_map names), int64; ties to the smaller list id."""
    idx, _ = exact_search(X, sqn, cent, _row_sqnorm(cent), 1, q_map=q_map)
    return idx[:, 0].long().clamp_(min=0)      # (-1 only for a row whose distances are all NaN)


def probe_lists(cent, n_probe):
    """int32 [n_lists, n_probe]: each list first, then the n_probe - 1 lists of nearest centroid."""
    n_lists = int(cent.shape[0])
    device = cent.device
    own = torch.arange(n_lists, dtype=torch.int32, device=device)[:, None]
    if n_probe >= n_lists:
        rest = torch.arange(n_lists, dtype=torch.int32, device=device).repeat(n_lists, 1)
        rest = rest[rest != own].view(n_lists, n_lists - 1)
        return torch.cat([own, rest], 1).contiguous()
    if n_probe == 1:
        return own.contiguous()
    csq = _row_sqnorm(cent)
    idx, _ = exact_search(cent, csq, cent, csq, n_probe - 1, flags=SELF)
    # a list with fewer than n_probe - 1 other lists cannot occur here (n_probe < n_lists); -1 is impossible
    return torch.cat([own, idx], 1).contiguous()


def _sync(device):
    torch.cuda.synchronize(device)


def check_n_refine(n_refine):
    """``n_refine`` as an int: the number of neighbour-of-neighbour passes.  A bool, a non-integer or a
    negative value is a ``ValueError``.  Needs no device."""
    if isinstance(n_refine, bool) or not isinstance(n_refine, int) or n_refine < 0:
        raise ValueError(f"n_refine must be a non-negative integer, the number of refinement passes "
                         f"(got {n_refine!r})")
    return n_refine


_D2_EMPTY = 0x7F7FFFFF   # the bits of FLT_MAX, the d2 of an empty slot
_IDX_EMPTY = 0x7FFFFFFF


def _list_keys(idx, d2):
    """int64 [n, k] keys (bits of d2) << 32 | index whose order is (d2, index) for d2 >= 0; an entry that is
    -1 gets the key of an empty slot, which follows every real one."""
    empty = idx < 0
    bits = d2.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    key = (bits << 32) | idx.long().clamp(min=0)
    return torch.where(empty, torch.full_like(key, (_D2_EMPTY << 32) | _IDX_EMPTY), key)


def _lists_of_keys(key):
    """(idx int32 [n, k], d2 [n, k]) of sorted ``_list_keys``: empty slots are (-1, FLT_MAX)."""
    low = key & 0xFFFFFFFF
    idx = torch.where(low == _IDX_EMPTY, torch.full_like(low, -1), low).to(torch.int32)
    d2 = (key >> 32).to(torch.int32).view(torch.float32)
    return idx.contiguous(), d2.contiguous()


def order_lists(X, idx):
    """Valid neighbour lists (idx, d2) from arbitrary indices idx int32 [n, k] into the prepared float32 rows
    X [n, nf]: each pair's float32 squared distance through ``mde_knn_ranks``' ``d2_out`` (the bits of the
    searches), rows ordered by (d2, index), self entries, entries outside [0, n) and repeated rows dropped,
    -1 slots trailing.  (The ranks that call also computes cost a pass over all pairs: this is for callers
    that hand in their own lists, not for the lists of a search, which come with their distances.)"""
    lib = _lib.load()
    n, nf, k = int(X.shape[0]), int(X.shape[1]), int(idx.shape[1])
    idx = idx.to(torch.int32).contiguous()
    ranks = torch.empty((n, k), dtype=torch.int32, device=X.device)
    d2 = torch.empty((n, k), dtype=torch.float32, device=X.device)
    work = _lib.work_buffer(lib.mde_knn_ranks_work_bytes, n, n, k, 0, device=X.device)
    _lib.check(lib.mde_knn_ranks(n, n, nf, _lib.ptr(X), _lib.ptr(X), 1, k, _lib.ptr(idx), 0, _lib.ptr(ranks),
                                 _lib.ptr(d2), _lib.ptr(work), _lib.stream_ptr(X.device)))
    rows = torch.arange(n, dtype=torch.int32, device=X.device)[:, None]
    idx = torch.where((idx < 0) | (idx >= n) | (idx == rows), torch.full_like(idx, -1), idx)
    key = torch.sort(_list_keys(idx, d2), 1).values
    repeat = torch.zeros_like(key, dtype=torch.bool)
    repeat[:, 1:] = key[:, 1:] == key[:, :-1]          # a row listed twice has one distance: adjacent keys
    key = torch.sort(torch.where(repeat, torch.full_like(key, (_D2_EMPTY << 32) | _IDX_EMPTY), key), 1).values
    return _lists_of_keys(key)


def reverse_lists(idx, d2, cap=None):
    """int32 [n, cap]: for every row t, among the rows j that list t (idx[j, s] == t), the ``cap`` (default
    k) with the smallest (d2[j, s], j), in that order, -1 padded.  One stable sort of the n k entries by
    (t, d2) -- they start in j order -- and offsets; d2 >= 0."""
    n, k = int(idx.shape[0]), int(idx.shape[1])
    cap = k if cap is None else int(cap)
    device = idx.device
    rev = torch.full((n, cap), -1, dtype=torch.int32, device=device)
    target = idx.reshape(-1).long()
    listed = target >= 0
    bits = d2.contiguous().view(torch.int32).reshape(-1).long() & 0xFFFFFFFF
    source = torch.arange(n, dtype=torch.int64, device=device).repeat_interleave(k)[listed]
    key = ((target << 32) | bits)[listed]
    key, order = torch.sort(key, stable=True)
    target = key >> 32
    first = torch.zeros(n + 1, dtype=torch.int64, device=device)
    first[1:] = torch.cumsum(torch.bincount(target, minlength=n), 0)
    place = torch.arange(key.shape[0], dtype=torch.int64, device=device) - first[target]
    keep = place < cap
    rev[target[keep], place[keep]] = source[order][keep].to(torch.int32)
    return rev


def refine_lists(X, idx, d2=None, n_iters=1, sqn=None, evaluated=None):
    """``n_iters`` neighbour-of-neighbour passes (``mde_knn_refine``, csrc/mde_ann_refine.hip) over the
    neighbour lists idx int32 [n, k] / d2 [n, k] of the prepared float32 rows X [n, nf], at any n.

    Each row's valid entries ascend by (d2, index), -1 slots trail, no row lists itself or another twice;
    with ``d2=None`` the lists are first put into that form by ``order_lists``.  A pass offers every row its
    reverse neighbours (``reverse_lists``) and the lists of its forward and reverse neighbours, and keeps the
    k smallest under (d2, index): entries only move earlier, every distance is the float32 value of the
    searches, an exact list stays as it is.  Returns (idx, d2, changed): ``changed`` is the list of
    per-pass counts of rows whose list changed; the passes stop early after one that changes none.
    ``evaluated``, when a list, receives the number of distances each pass computed."""
    lib = _lib.load()
    n, nf, k = int(X.shape[0]), int(X.shape[1]), int(idx.shape[1])
    device = X.device
    if d2 is None:
        idx, d2 = order_lists(X, idx)
    idx, d2 = idx.to(torch.int32).contiguous(), d2.to(torch.float32).contiguous()
    if sqn is None:
        sqn = _row_sqnorm(X)
    changed = []
    work = _lib.work_buffer(lib.mde_knn_refine_work_bytes, n, k, device=device)
    count = torch.zeros(1, dtype=torch.int32, device=device)
    for _ in range(check_n_refine(n_iters)):
        rev = reverse_lists(idx, d2)
        idx_new, d2_new = torch.empty_like(idx), torch.empty_like(d2)
        _lib.check(lib.mde_knn_refine(n, nf, _lib.ptr(X), _lib.ptr(sqn), k, _lib.ptr(idx), _lib.ptr(d2),
                                      _lib.ptr(rev), _lib.ptr(idx_new), _lib.ptr(d2_new), _lib.ptr(count),
                                      _lib.ptr(work), _lib.stream_ptr(device)))
        idx, d2 = idx_new, d2_new
        changed.append(int(count.item()))
        if evaluated is not None:
            evaluated.append(int(work[:8].view(torch.int64).item()))
        if changed[-1] == 0:
            break
    return idx, d2, changed


def knn_lists(X, k, n_lists=None, n_probe=None, seed=0, timings=None, n_refine=0):
    """Approximate directed neighbour lists (idx [n, k] int32, d2 [n, k]) of a dense float32 [n, nf] on the
    GPU, in the caller's row order.  Rows with fewer than k candidates get -1 slots.  ``n_refine`` passes of
    ``refine_lists`` follow the scan (0: none, and nothing else is launched).

    ``timings``, when a dict, receives the seconds of each stage (synchronising between them) and the
    sizes of the lists, the tile count and the load imbalance of the scan; with ``n_refine`` also the
    ``"refine"`` lap, the rows each pass changed (``"refine_changed"``) and the distances it evaluated
    (``"refine_evaluated"``)."""
    n, nf = int(X.shape[0]), int(X.shape[1])
    device = X.device
    n_lists, n_probe = resolve_params(n, n_lists, n_probe)
    n_refine = check_n_refine(n_refine)
    timed = timings is not None
    clock = _Clock(device, timed)
    sqn = _row_sqnorm(X)
    cent = kmeans(X, sqn, n_lists, seed)
    clock.lap(timings, "kmeans")
    labels = assign(X, sqn, cent)
    perm, offsets = _sort_by_list(labels, n_lists)
    perm = perm.to(torch.int32).contiguous()
    clock.lap(timings, "assign")
    probe = probe_lists(cent, n_probe)
    offsets_h, probe_h = offsets.cpu(), probe.long().cpu()
    tiles_h, cost = tile_list(offsets_h, probe_h)
    tiles = tiles_h.to(device)
    clock.lap(timings, "probe")
    idx, d2 = search(X, sqn, X, sqn, k, offsets, probe, tiles, q_map=perm, b_map=perm, flags=SELF | SCATTER)
    clock.lap(timings, "scan")
    if n_refine:
        evaluated = [] if timed else None
        idx, d2, changed = refine_lists(X, idx, d2, n_iters=n_refine, sqn=sqn, evaluated=evaluated)
        clock.lap(timings, "refine")
        if timed:
            timings.update(refine_changed=changed, refine_evaluated=evaluated)
    if timed:
        sizes = offsets_h[1:] - offsets_h[:-1]
        timings.update(n_lists=n_lists, n_probe=n_probe, list_sizes=sizes, tiles=int(tiles_h.shape[0]),
                       candidate_pairs=int((sizes * sizes[probe_h].sum(1)).sum()),
                       imbalance=imbalance(cost, _slots(device, k)))
    return idx, d2


def _slots(device, k):
    """Workgroups of the scan resident at once: four per CU by registers, fewer when the LDS binds."""
    lds = 4 * (64 * 33 * 2 + 64 * 65 + 256) + 64 * k * 8
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return cus * max(1, min(4, (160 * 1024) // lds))


class _Clock(object):
    def __init__(self, device, on):
        import time
        self._time, self._device, self._on = time.perf_counter, device, on
        self._t = self._time() if on else 0.0

    def lap(self, out, name):
        if not self._on:
            return
        _sync(self._device)
        t = self._time()
        out[name] = t - self._t
        self._t = t


def sampled_recall(X, idx, k, n_samples=1000, seed=0):
    """Estimated recall@k of neighbour lists idx [n, k] (int32, -1 = empty): the share of the exact k
    nearest neighbours of ``n_samples`` seeded random rows found in their lists.  The exact lists come
    from the query-against-base kernel."""
    n = int(X.shape[0])
    g = torch.Generator(device=X.device)
    g.manual_seed(int(seed) + 1)
    m = min(n, int(n_samples))
    rows = torch.randperm(n, generator=g, device=X.device)[:m].to(torch.int32).contiguous()
    sqn = _row_sqnorm(X)
    truth, _ = exact_search(X, sqn, X, sqn, k, q_map=rows, flags=SELF)
    got = idx[rows.long()]
    valid = truth >= 0
    hit = (truth[:, :, None] == got[:, None, :]).any(2) & valid
    return float(hit.sum().item()) / max(1, int(valid.sum().item()))
