"""Record scikit-learn's trustworthiness and continuity of a small embedding, on the CPU.

    python tests/golden/make_quality.py

writes ``quality.npz`` next to this file: integer-grid data [150, 8] and an integer-grid embedding [150, 2],
``n_neighbors`` and the two scores of ``sklearn.manifold.trustworthiness`` (continuity is the same function
with the two spaces swapped).  scikit-learn is needed here only; no test imports it.

The input is chosen so that nothing is left to rounding or to a tie rule: every row's 149 squared distances
are distinct and non-zero in both spaces (asserted below), and every float32 product and sum on them is exact
(norms below 2^23, sums below 2^24; the translation of a Euclidean search moves integers to integers).  The
ranks are therefore unambiguous, the GPU's must equal sklearn's, and both sides evaluate the same rational
number in float64: the tests compare to 1e-12.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "quality.npz")
SEED, N, NF, D, N_NEIGHBORS = 33, 150, 8, 2, 7


def inputs():
    rng = np.random.default_rng(SEED)
    data = rng.integers(0, 1024, (N, NF))
    X = rng.integers(0, 2048, (N, D))
    return data, X


def squared_distances(A):
    """Exact int64 squared distances of the rows of an integer matrix."""
    A = np.asarray(A, dtype=np.int64)
    diff = A[:, None, :] - A[None, :, :]
    return (diff * diff).sum(-1)


def assert_unambiguous(A):
    d2 = squared_distances(A)
    n = d2.shape[0]
    off = d2[~np.eye(n, dtype=bool)].reshape(n, n - 1)
    assert (off > 0).all(), "duplicate rows"
    assert all(np.unique(row).size == n - 1 for row in off), "tied distances in a row"
    norms = (np.asarray(A, dtype=np.int64) ** 2).sum(1)
    assert norms.max() < 2 ** 23 and 2 * norms.max() < 2 ** 24, "float32 arithmetic would round"


def main():
    from sklearn.manifold import trustworthiness
    data, X = inputs()
    assert_unambiguous(data)
    assert_unambiguous(X)
    t = trustworthiness(data.astype(np.float64), X.astype(np.float64), n_neighbors=N_NEIGHBORS)
    c = trustworthiness(X.astype(np.float64), data.astype(np.float64), n_neighbors=N_NEIGHBORS)
    np.savez(OUT, data=data.astype(np.int32), X=X.astype(np.int32), n_neighbors=np.int32(N_NEIGHBORS),
             trustworthiness=np.float64(t), continuity=np.float64(c))
    print("trustworthiness %r continuity %r -> %s (%d bytes)" % (float(t), float(c), OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
