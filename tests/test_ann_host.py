"""Host logic of the approximate k-NN search (pymde_amd/ann.py, recipes): parameter resolution and
validation, the tile list and its load-balance figure, the recipes' ``approximate_neighbors`` values.
No GPU needed."""
import pytest
import torch

from pymde_amd import ann, recipes


def test_default_parameters():
    assert ann.resolve_params(200000) == (447, 32)
    assert ann.resolve_params(1000000) == (1000, 32)
    assert ann.resolve_params(20000) == (141, 32)
    assert ann.resolve_params(100) == (10, 10)          # n_probe = min(32, n_lists)
    assert ann.resolve_params(20000, n_lists=50) == (50, 32)
    assert ann.resolve_params(20000, n_probe=8) == (141, 8)


def test_every_list_probed_and_caps():
    assert ann.resolve_params(20000, n_lists=141, n_probe=141) == (141, 141)
    assert ann.resolve_params(20000, n_lists=141, n_probe=1000) == (141, 141)
    assert ann.resolve_params(50, n_lists=80, n_probe=2) == (50, 2)      # at most n lists
    assert ann.resolve_params(20000, n_lists=5000, n_probe=65) == (5000, 65)


@pytest.mark.parametrize("kw", [{"n_lists": 0}, {"n_probe": 0}, {"n_lists": -3}, {"n_probe": -1},
                                {"n_lists": 500, "n_probe": 66}])
def test_invalid_parameters(kw):
    with pytest.raises(ValueError):
        ann.resolve_params(20000, **kw)


def test_tile_list_covers_every_position_heaviest_first():
    sizes = torch.tensor([130, 0, 64, 1, 200, 7])
    offsets = torch.zeros(7, dtype=torch.int64)
    offsets[1:] = torch.cumsum(sizes, 0)
    probe = torch.tensor([[0, 4], [1, 0], [2, 3], [3, 2], [4, 0], [5, 1]])
    tiles, cost = ann.tile_list(offsets, probe)
    lo, hi, lst = tiles[:, 0], tiles[:, 1], tiles[:, 2]
    assert bool((hi > lo).all()) and bool((hi - lo <= 64).all())
    covered = torch.zeros(int(offsets[-1]), dtype=torch.int64)
    for a, b, l in tiles.tolist():
        assert offsets[l] <= a and b <= offsets[l + 1]
        covered[a:b] += 1
    assert bool((covered == 1).all())
    assert cost.tolist() == sorted(cost.tolist(), reverse=True)
    expect = {0: 330, 2: 65, 3: 65, 4: 330, 5: 7}
    assert all(int(c) == expect[int(l)] for c, l in zip(cost, lst))
    # ties keep list order (stable): list 0's tiles before list 4's
    assert lst[:3].tolist() == [0, 0, 0] and lst[3:7].tolist() == [4, 4, 4, 4]


def test_imbalance():
    assert ann.imbalance(torch.tensor([5, 5, 5, 5]), 2) == 1.0
    assert ann.imbalance(torch.tensor([8, 1, 1]), 2) == pytest.approx(8 / 5)
    assert ann.imbalance(torch.tensor([0, 0]), 4) == 1.0
    assert ann.imbalance(torch.tensor([3]), 100) == 1.0


def test_recipe_options():
    assert recipes._approximate_options(False) == {}
    assert recipes._approximate_options(None) == {}
    assert recipes._approximate_options(True) == {"approximate": True}
    assert recipes._approximate_options({"n_lists": 10, "n_probe": 3}) == {"approximate": True, "n_lists": 10,
                                                                            "n_probe": 3}
    with pytest.raises(ValueError):
        recipes._approximate_options({"nprobe": 3})
    with pytest.raises(ValueError):
        recipes._approximate_options("yes")
