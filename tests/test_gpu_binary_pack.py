"""binary.pack / from_packbits on the GPU (mde_bits_pack, mde_bits_pack_csr): the words, the counts and the padding
bits at every width around the 32- and 64-bit seams, from every input form, and the rows that are not binary."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from pymde_amd import binary

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 257]
NFS = [1, 31, 32, 33, 64, 65, 1000]


def _random_bits(n, nf, seed=0):
    B = np.random.default_rng(seed + 1000 * n + nf).random((n, nf)) < 0.4
    if n > 2:
        B[1] = False                       # an all-zero row
        B[2] = True                        # and a full one: every bit below n_features, none above
    return B


def _check(bits, B):
    n, nf = B.shape
    assert bits.shape == (n, nf) and bits.words.dtype == torch.int32 and bits.counts.dtype == torch.int32
    assert tuple(bits.words.shape) == (n, (nf + 31) // 32)
    got = bits.unpack()
    assert got.dtype == torch.bool and tuple(got.shape) == (n, nf)
    assert np.array_equal(got.cpu().numpy(), B)
    assert np.array_equal(bits.counts.cpu().numpy(), B.sum(1))
    if nf % 32:                            # every bit at or beyond n_features is zero
        last = bits.words[:, -1].cpu().numpy().view(np.uint32)
        assert not (last >> np.uint32(nf % 32)).any()


@pytest.mark.parametrize("nf", NFS)
@pytest.mark.parametrize("n", NS)
def test_pack_round_trip_from_every_dtype(n, nf):
    B = _random_bits(n, nf)
    words = None
    for data in (B, B.astype(np.float32), B.astype(np.int8), torch.from_numpy(B.astype(np.int64))):
        bits = binary.pack(data)
        _check(bits, B)
        if words is None:
            words = bits.words
        assert torch.equal(bits.words, words)
    assert bits.distance == "jaccard" and binary.pack(B, "Tanimoto").distance == "jaccard"
    ham = bits.with_distance("hamming")
    assert ham.distance == "hamming" and ham.words.data_ptr() == bits.words.data_ptr()


def test_pack_from_a_device_tensor_and_float64():
    B = _random_bits(65, 100)
    _check(binary.pack(torch.from_numpy(B).cuda()), B)
    _check(binary.pack(B.astype(np.float64)), B)
    _check(binary.pack(torch.from_numpy(B.astype(np.float16)).cuda()), B)


@pytest.mark.parametrize("bad", [2.0, 0.5, float("nan"), -1.0])
def test_a_value_that_is_not_binary_names_its_row(bad):
    X = _random_bits(257, 65).astype(np.float32)
    X[200, 64] = bad
    X[131, 3] = bad
    with pytest.raises(ValueError, match=r"row 131 .*data != 0"):
        binary.pack(X)
    with pytest.raises(ValueError, match="row 131 "):
        binary.pack(sp.csr_matrix(np.nan_to_num(X, nan=7.0)))


def test_values_that_float32_would_round_to_binary_are_refused():
    X = _random_bits(10, 40).astype(np.float64)
    X[7, 0] = 1e-60
    with pytest.raises(ValueError, match="row 7 "):
        binary.pack(X)
    X[7, 0] = 1.0 + 1e-12
    with pytest.raises(ValueError, match="row 7 "):
        binary.pack(X)
    Y = _random_bits(10, 40).astype(np.int64)
    Y[4, 39] = 2 ** 40
    with pytest.raises(ValueError, match="row 4 "):
        binary.pack(Y)


@pytest.mark.parametrize("n,nf", [(1, 1), (65, 33), (257, 1000), (64, 64)])
def test_sparse_input_gives_the_words_of_the_dense_input(n, nf):
    B = _random_bits(n, nf)
    want = binary.pack(B)
    S = sp.csr_matrix(B.astype(np.float32))
    coo = torch.from_numpy(B.astype(np.float32)).to_sparse()
    for data in (S, S.tocsc(), S.tocoo(), sp.csr_matrix(B), coo, coo.to_sparse_csr()):
        got = binary.pack(data)
        assert torch.equal(got.words, want.words) and torch.equal(got.counts, want.counts)
        assert got.shape == (n, nf)


def test_sparse_duplicates_that_sum_past_one_are_not_binary():
    S = sp.coo_matrix((np.ones(3, np.float32), ([0, 2, 2], [1, 5, 5])), shape=(4, 9))
    with pytest.raises(ValueError, match="row 2 "):
        binary.pack(S)


def test_pack_csr_kernel_on_raw_arrays():
    """mde_bits_pack_csr itself: a duplicate entry sets its bit once, a stored zero sets nothing, and a column
    outside [0, nf) or a value other than 0 / 1 makes the row bad."""
    from pymde_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")

    def run(indptr, indices, values, n, nf):
        indptr = torch.tensor(indptr, dtype=torch.int64, device=dev)
        indices = torch.tensor(indices, dtype=torch.int32, device=dev)
        values = torch.tensor(values, dtype=torch.float32, device=dev)
        nw = (nf + 31) // 32
        words = torch.full((n, nw), -1, dtype=torch.int32, device=dev)
        counts = torch.full((n,), -1, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.mde_bits_pack_csr(n, nf, int(indices.shape[0]), _lib.ptr(indptr), _lib.ptr(indices),
                                         _lib.ptr(values), _lib.ptr(words), _lib.ptr(counts), _lib.ptr(bad),
                                         _lib.stream_ptr(dev)))
        return words.cpu().numpy().view(np.uint32), counts.cpu().numpy(), int(bad.item())

    words, counts, bad = run([0, 3, 3, 5], [33, 33, 0, 2, 40], [1, 1, 0, 1, 1], 3, 41)
    assert bad == 2 ** 31 - 1
    assert words.tolist() == [[0, 2], [0, 0], [4, 256]] and counts.tolist() == [1, 0, 2]
    assert run([0, 1, 2], [3, 41], [1, 1], 2, 41)[2] == 1
    assert run([0, 1, 2], [-1, 4], [1, 1], 2, 41)[2] == 0
    assert run([0, 1, 2], [3, 4], [1, 2], 2, 41)[2] == 1


@pytest.mark.parametrize("bitorder", ["big", "little"])
@pytest.mark.parametrize("n,nf", [(1, 1), (63, 31), (65, 33), (64, 64), (257, 1000), (5, 2048)])
def test_from_packbits(n, nf, bitorder):
    B = _random_bits(n, nf)
    packed = np.packbits(B, axis=1, bitorder=bitorder)
    bits = binary.from_packbits(packed, nf, bitorder=bitorder)
    _check(bits, np.unpackbits(packed, axis=1, count=nf, bitorder=bitorder).astype(bool))
    assert torch.equal(bits.words, binary.pack(B).words)
    assert binary.from_packbits(torch.from_numpy(packed).cuda(), nf, "hamming", bitorder).distance == "hamming"


@pytest.mark.parametrize("bitorder", ["big", "little"])
def test_from_packbits_in_row_chunks(bitorder, monkeypatch):
    """The conversion takes the rows a chunk at a time: chunks of 3 rows give the bits of one chunk, and a bit
    beyond n_features in a later chunk names its row."""
    B = _random_bits(65, 33)
    packed = np.packbits(B, axis=1, bitorder=bitorder)
    want = binary.from_packbits(packed, 33, bitorder=bitorder)
    monkeypatch.setattr(binary, "_PACKBITS_CHUNK_BYTES", 3 * 8)        # 3 rows of two words
    got = binary.from_packbits(packed, 33, bitorder=bitorder)
    assert torch.equal(got.words, want.words) and torch.equal(got.counts, want.counts)
    _check(got, B)
    bad = np.packbits(np.concatenate([B, np.zeros((65, 7), bool)], 1), axis=1, bitorder=bitorder)
    flip = np.zeros((65, 40), bool)
    flip[50, 36] = True
    bad |= np.packbits(flip, axis=1, bitorder=bitorder)
    with pytest.raises(ValueError, match="row 50"):
        binary.from_packbits(bad, 33, bitorder=bitorder)


@pytest.mark.parametrize("bitorder", ["big", "little"])
def test_from_packbits_refuses_bits_beyond_n_features(bitorder):
    B = np.zeros((6, 40), bool)
    B[4, 37] = True
    packed = np.packbits(B, axis=1, bitorder=bitorder)
    binary.from_packbits(packed, 38, bitorder=bitorder)
    with pytest.raises(ValueError, match="row 4"):
        binary.from_packbits(packed, 37, bitorder=bitorder)
