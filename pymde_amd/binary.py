"""Bit-packed binary data: the Jaccard (Tanimoto) and Hamming distances on packed rows (csrc/mde_bits.hip,
DESIGN section 6v).  The reference has no binary distance (its k-NN is Euclidean); the definitions are those of
``scipy.spatial.distance``.

A ``BitMatrix`` is a kind of input that carries its own distance, the way a ``Graph`` carries its shortest-path
metric: ``metric=`` stays at its default beside it, and the name tables of ``pymde_amd.metrics`` do not know the
binary distances.  ``pack`` builds one from a 0/1 matrix (dense or sparse), ``from_packbits`` from the bytes of
``np.packbits(..., axis=1)``.  A matrix of ``n_features`` bits per row takes ``ceil(n_features / 32)`` int32 words
per row on the GPU -- a 32nd of its float32 form.

With ``a``, ``b`` the numbers of ones of two rows and ``t`` the number they share:

  * ``"hamming"`` -- ``(a + b - 2 t) / n_features``;
  * ``"jaccard"`` (alias ``"tanimoto"``) -- ``(a + b - 2 t) / (a + b - t)``, and 0 for two empty rows,

each one float32 division of exact integers, so a pair has the same bits wherever it is computed.
"""
import numpy as np
import torch

from pymde_amd import _lib
from pymde_amd import metrics as _metrics
from pymde_amd import sparse as _sparse
from pymde_amd import util

JACCARD, HAMMING = "jaccard", "hamming"
DISTANCES = (JACCARD, HAMMING)
ALIASES = {"tanimoto": JACCARD}
KINDS = {JACCARD: 0, HAMMING: 1}           # `kind` of mde_bits_knn / mde_bits_pair_distances
MAX_FEATURES = 2 ** 24                     # every count below it is exact in float32
_PACK_CHUNK_BYTES = 1 << 28                # the float32 staging copy of `pack` is made this many bytes at a time


def resolve_distance(distance):
    """``"jaccard"`` or ``"hamming"`` for a name or alias (case-insensitive); ``ValueError`` for anything else.
    Needs no device."""
    name = distance.strip().lower() if isinstance(distance, str) else distance
    name = ALIASES.get(name, name) if isinstance(name, str) else name
    if not isinstance(name, str) or name not in DISTANCES:
        raise ValueError(f"unknown binary distance {distance!r}; the distances of a BitMatrix are "
                         f"{', '.join(DISTANCES)} (alias: tanimoto)")
    return name


def is_bits(data):
    return isinstance(data, BitMatrix)


def check_metric(metric):
    """A ``BitMatrix`` carries its own distance: only the default ``metric=`` may accompany it."""
    if _metrics.resolve(metric) != _metrics.EUCLIDEAN:
        raise ValueError(f"metric={metric!r} applies to float data matrices; a BitMatrix carries its own distance "
                         "(BitMatrix.distance, changed by with_distance)")


def refuse(data, who, instead=None):
    """``ValueError`` when ``data`` is a ``BitMatrix``: ``who`` has no form on packed bits.  Needs no device."""
    if isinstance(data, BitMatrix):
        raise ValueError(f"{who} does not take a BitMatrix (bit-packed binary data are served by the exact "
                         "neighbour searches, recipes.distances and the recipes built on them)"
                         + (f"; {instead}" if instead else ""))


class BitMatrix(object):
    """A binary data matrix on the GPU, 32 features to a word, that names the distance it is compared by.

    ``words`` int32 [n, ceil(n_features / 32)] (feature ``f`` is bit ``f & 31`` of word ``f >> 5``; every padding
    bit is zero), ``counts`` int32 [n] (the ones of every row), ``n_features``, ``distance``; ``shape`` is
    ``(n, n_features)``.  Build one with ``pack`` or ``from_packbits``."""

    def __init__(self, words, counts, n_features, distance=JACCARD):
        n_features = int(n_features)
        if not 1 <= n_features < MAX_FEATURES:
            raise ValueError(f"a BitMatrix has between 1 and 2^24 - 1 features (got {n_features})")
        nw = (n_features + 31) // 32
        if (not isinstance(words, torch.Tensor) or words.dtype != torch.int32 or words.dim() != 2
                or int(words.shape[1]) != nw):
            raise ValueError(f"`words` must be an int32 tensor [n, {nw}] for {n_features} features")
        if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.dim() != 1
                or int(counts.shape[0]) != int(words.shape[0]) or counts.device != words.device):
            raise ValueError("`counts` must be an int32 tensor [n] on the device of `words`")
        self.words = words.contiguous()
        self.counts = counts.contiguous()
        self.n_features = n_features
        self.distance = resolve_distance(distance)

    @property
    def shape(self):
        return (int(self.words.shape[0]), self.n_features)

    @property
    def device(self):
        return self.words.device

    @property
    def kind(self):
        return KINDS[self.distance]

    def __len__(self):
        return int(self.words.shape[0])

    def __repr__(self):
        return f"BitMatrix({self.shape[0]} x {self.n_features}, distance='{self.distance}', device='{self.device}')"

    def with_distance(self, distance):
        """The same rows (the words are shared, not copied) compared by ``distance``."""
        return BitMatrix(self.words, self.counts, self.n_features, distance)

    def to(self, device):
        device = torch.device(device)
        if device == self.device:
            return self
        return BitMatrix(self.words.to(device), self.counts.to(device), self.n_features, self.distance)

    def unpack(self):
        """The bool [n, n_features] tensor of the bits, on the device of the words."""
        shifts = torch.arange(32, dtype=torch.int32, device=self.device)
        bits = (self.words.unsqueeze(2) >> shifts) & 1
        return bits.reshape(self.shape[0], -1)[:, :self.n_features].to(torch.bool)


def _not_binary(row):
    raise ValueError(f"binary data must hold only 0 and 1: row {row} holds another value (NaN counts as one); "
                     "pass `data != 0` to treat every non-zero entry as a one")


def _pack_device(n_features, device):
    if not 1 <= int(n_features) < MAX_FEATURES:
        raise ValueError(f"a BitMatrix has between 1 and 2^24 - 1 features (got {int(n_features)})")
    return util.require_cuda_device(util.get_default_device() if device is None else device)


def _as_float32(block, device):
    """The float32 copy on ``device`` of a block of rows, with NaN where the copy would hide a value that is
    neither 0 nor 1 (a float64 that rounds to 0 or 1)."""
    block = block.to(device)
    if block.dtype == torch.float32:
        return block.contiguous()
    if block.is_complex():
        raise ValueError("binary data must be real")
    out = block.to(torch.float32)
    if block.dtype == torch.float64:
        out = torch.where(out.to(torch.float64) == block, out, torch.full_like(out, float("nan")))
    return out.contiguous()


def pack(data, distance=JACCARD, device=None):
    """The ``BitMatrix`` of a binary data matrix [n, n_features]: a dense ``np.ndarray`` / ``torch.Tensor`` of bool
    or any numeric dtype, or a sparse matrix (scipy sparse of any format, torch sparse COO / CSR).  Every entry --
    of a sparse matrix, every stored value after duplicates are summed -- must be exactly 0 or 1; anything else,
    NaN included, is a ``ValueError`` naming the first such row (``data != 0`` makes any matrix binary).  Dense
    data are packed by ``mde_bits_pack`` from a float32 staging copy made 256 MB at a time, sparse data by
    ``mde_bits_pack_csr``."""
    distance = resolve_distance(distance)
    if isinstance(data, BitMatrix):
        return data.with_distance(distance) if device is None else data.to(device).with_distance(distance)
    lib_sparse = _sparse.is_sparse(data)
    if not lib_sparse and not isinstance(data, torch.Tensor):
        data = torch.as_tensor(np.asarray(data))
    if len(data.shape) != 2:
        raise ValueError(f"`data` must be a matrix [n, n_features] (got shape {tuple(data.shape)})")
    n, nf = int(data.shape[0]), int(data.shape[1])
    if n < 1:
        raise ValueError("`data` needs at least one row")
    if device is None and isinstance(data, torch.Tensor) and data.is_cuda:
        device = data.device
    device = _pack_device(nf, device)
    nw = (nf + 31) // 32
    lib = _lib.load()
    words = torch.empty((n, nw), dtype=torch.int32, device=device)
    counts = torch.empty(n, dtype=torch.int32, device=device)
    bad = torch.empty(1, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        if lib_sparse:
            csr = _sparse.to_device_csr(data, device)
            _lib.check(lib.mde_bits_pack_csr(n, nf, csr.nnz, _lib.ptr(csr.indptr), _lib.ptr(csr.indices),
                                             _lib.ptr(csr.values), _lib.ptr(words), _lib.ptr(counts), _lib.ptr(bad),
                                             _lib.stream_ptr(device)))
            first = int(bad.item())
            if first != 2 ** 31 - 1:
                _not_binary(first)
        else:
            data = data.detach()
            step = max(1, _PACK_CHUNK_BYTES // (4 * nf))
            for r0 in range(0, n, step):
                r1 = min(n, r0 + step)
                block = _as_float32(data[r0:r1], device)
                _lib.check(lib.mde_bits_pack(r1 - r0, nf, _lib.ptr(block), _lib.ptr(words[r0:r1]),
                                             _lib.ptr(counts[r0:r1]), _lib.ptr(bad), _lib.stream_ptr(device)))
                first = int(bad.item())
                if first != 2 ** 31 - 1:
                    _not_binary(r0 + first)
    return BitMatrix(words, counts, nf, distance)


_PACKBITS_CHUNK_BYTES = 1 << 25            # `from_packbits` converts this many bytes of rows at a time
_BYTE_REVERSE = [int(f"{b:08b}"[::-1], 2) for b in range(256)]
_BYTE_POPCOUNT = [bin(b).count("1") for b in range(256)]


def check_packbits_shape(shape, n_features, bitorder="big"):
    """The argument errors of ``from_packbits`` that need no device."""
    if bitorder not in ("big", "little"):
        raise ValueError(f"bitorder must be 'big' or 'little' (got {bitorder!r})")
    n_features = int(n_features)
    if not 1 <= n_features < MAX_FEATURES:
        raise ValueError(f"a BitMatrix has between 1 and 2^24 - 1 features (got {n_features})")
    if len(shape) != 2 or int(shape[1]) != (n_features + 7) // 8:
        raise ValueError(f"`packed` must be uint8 [n, {(n_features + 7) // 8}] for {n_features} features, the "
                         f"output of np.packbits(bits, axis=1) (got shape {tuple(shape)})")
    if int(shape[0]) < 1:
        raise ValueError("`packed` needs at least one row")


def from_packbits(packed, n_features, distance=JACCARD, bitorder="big", device=None):
    """The ``BitMatrix`` of the uint8 [n, ceil(n_features / 8)] output of ``np.packbits(bits, axis=1,
    bitorder=bitorder)``, the form in which fingerprint toolkits hand their bits over: ``unpack()`` of the result
    equals ``np.unpackbits(packed, axis=1, count=n_features, bitorder=bitorder)``.  A set bit at or beyond
    ``n_features`` is a ``ValueError``.  The conversion is a few torch operations on the GPU, on 32 MB of rows at a
    time (its table lookups take 8 bytes of index per byte)."""
    distance = resolve_distance(distance)
    if not isinstance(packed, torch.Tensor):
        packed = torch.as_tensor(np.asarray(packed))
    if packed.dtype != torch.uint8:
        raise ValueError(f"`packed` must be uint8, the output of np.packbits (got dtype {packed.dtype})")
    check_packbits_shape(packed.shape, n_features, bitorder)
    n, nf = int(packed.shape[0]), int(n_features)
    if device is None and packed.is_cuda:
        device = packed.device
    device = _pack_device(nf, device)
    nw = (nf + 31) // 32
    reverse = torch.tensor(_BYTE_REVERSE, dtype=torch.uint8, device=device)
    popcount = torch.tensor(_BYTE_POPCOUNT, dtype=torch.int32, device=device)
    padded = torch.zeros((n, 4 * nw), dtype=torch.uint8, device=device)
    counts = torch.empty(n, dtype=torch.int32, device=device)
    tail, nb = nf % 8, int(packed.shape[1])
    # the table lookups index with int64, 8 bytes per byte of input: rows are taken 32 MB of bytes at a time
    step = max(1, _PACKBITS_CHUNK_BYTES // (4 * nw))
    for r0 in range(0, n, step):
        block = packed[r0:r0 + step].to(device)
        if bitorder == "big":    # feature 8 b + j is bit 7 - j of byte b: reverse the bits of every byte
            block = reverse[block.to(torch.int64)]
        beyond = block[:, -1] >> tail if tail else None
        if beyond is not None and bool(beyond.any()):
            raise ValueError(f"`packed` holds set bits at or beyond n_features = {nf} (first in row "
                             f"{r0 + int(beyond.nonzero()[0])})")
        padded[r0:r0 + step, :nb] = block
        counts[r0:r0 + step] = popcount[block.to(torch.int64)].sum(1, dtype=torch.int32)
    # little-endian bytes: feature f = 8 b + j is bit 8 (b & 3) + j of word b >> 2, which is bit f & 31 of word f >> 5
    words = padded.view(torch.int32).contiguous()
    return BitMatrix(words, counts, nf, distance)


def check_pair(queries, data):
    """Two ``BitMatrix`` arguments of a cross search must agree on ``n_features`` and ``distance``."""
    if not (isinstance(queries, BitMatrix) and isinstance(data, BitMatrix)):
        raise ValueError("a BitMatrix is searched against a BitMatrix: pack both arguments (binary.pack)")
    if queries.n_features != data.n_features:
        raise ValueError(f"the two BitMatrix arguments have {queries.n_features} and {data.n_features} features; "
                         "they must agree")
    if queries.distance != data.distance:
        raise ValueError(f"the two BitMatrix arguments are compared by '{queries.distance}' and '{data.distance}'; "
                         "they must agree (with_distance)")


def knn_lists(queries, data, k, self_join=False, slices=0):
    """``(idx [n_q, k] int32, dist [n_q, k] float32)`` of ``mde_bits_knn``: for every row of ``queries`` its ``k``
    nearest rows of ``data`` (two ``BitMatrix`` on one GPU, or one and ``self_join``) ordered by (distance, index);
    empty slots hold -1 / FLT_MAX."""
    n_q, n_c = queries.shape[0], data.shape[0]
    device = data.device
    lib = _lib.load()
    idx = torch.empty((n_q, k), dtype=torch.int32, device=device)
    dist = torch.empty((n_q, k), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        work = _lib.work_buffer(lib.mde_bits_knn_work_bytes, n_q, n_c, k, slices, device=device)
        _lib.check(lib.mde_bits_knn(n_q, n_c, int(data.words.shape[1]), data.n_features, _lib.ptr(queries.words),
                                    _lib.ptr(queries.counts), _lib.ptr(data.words), _lib.ptr(data.counts),
                                    int(self_join), data.kind, k, slices, _lib.ptr(idx), _lib.ptr(dist),
                                    _lib.ptr(work), _lib.stream_ptr(device)))
    return idx, dist


def pair_distances(bits, edges):
    """The distances of ``bits`` between its rows named by edges [p, 2] (int64, on its GPU), with the bits the
    search gives each pair (``mde_bits_pair_distances``); NaN for an endpoint outside ``[0, n)``."""
    out = torch.empty(edges.shape[0], dtype=torch.float32, device=bits.device)
    with torch.cuda.device(bits.device):
        _lib.check(_lib.load().mde_bits_pair_distances(bits.shape[0], int(bits.words.shape[1]), bits.n_features,
                                                       _lib.ptr(bits.words), _lib.ptr(bits.counts), edges.shape[0],
                                                       _lib.ptr(edges), bits.kind, _lib.ptr(out),
                                                       _lib.stream_ptr(bits.device)))
    return out
