"""The matrix of tests/data_sweep.py without a device: every cell of the coverage list is reached by a case (from the restated planner
alone), the reference can tell the contract's tree from sums in another order on every case's own inputs, and the references stay
small.  What the kernels compute at these shapes is tests/test_gpu_data_sweep.py."""
import time

import numpy as np
import pytest

import data_sweep as ds
from test_data_density_cpu import pairwise, recursive


def test_the_restated_planner_on_shapes_worked_out_by_hand():
    """Plans read off data_plan by hand: the mapping boundary, the grid cap (rounds double while groups x blocks > 2048 and more than
    one block is left), the depth cap, and the three shapes whose plans the existing GPU tests assert from describe()."""
    assert ds.plan(511, 5000) == ("obs", 8, 3, 511) and ds.plan(512, 5000) == ("lane", 1, 79, 8)
    assert ds.plan(50, 1000) == ("obs", 1, 4, 50) and ds.plan(50, 1000, "lane") == ("lane", 1, 16, 1)        # test_mapping_switch_after_creation...
    assert ds.plan(2048, 20001) == ("lane", 8, 40, 32) and ds.plan(2048, 20001, "obs") == ("obs", 128, 1, 2048)   # test_many_rounds_per_wave...
    assert ds.plan(1, 524288) == ("obs", 1, 2048, 1) and ds.plan(1, 524289) == ("obs", 2, 1025, 1)
    assert ds.plan(65536, 131073, "lane") == ("lane", 2048, 2, 1024) and ds.plan(65537, 131073, "lane") == ("lane", 4096, 1, 1025)
    assert ds.plan(64, 2 ** 30, "lane") == ("lane", 4096, 4096, 1)                                               # both caps at once
    assert ds.last_block(3000, 3001) == (2, 25, 2, 9, 56) and ds.last_block(1025, 524289, "obs") == (3, 1, 1, 1, 1)
    assert ds.last_block(16384, 2287) == (2, 111, 7, 15, 0) and ds.last_block(512, 256, "obs") == (4, 64, 1, 64, 0)


def test_every_cell_of_the_coverage_list_is_reached():
    missing = [name for name, ids in ds.coverage().items() if not ids]
    assert not missing, "no case reaches: " + "; ".join(missing)
    assert len(set(ds.CASES)) == len(ds.CASES)
    assert ds.LANE_DEEP in ds.CASES


def test_coverage_is_computed_not_assumed():
    """Without the cases that reach it, a cell is reported missing."""
    few = [c for c in ds.CASES if ds.plan(*c).rounds != ds.RMAX and ds.plan(*c).nblocks != 2048]
    cov = ds.coverage(few)
    assert not cov["obs: rounds 4096"] and not cov["lane: rounds 4096"] and not cov["obs: nblocks 2048"] and not cov["lane: nblocks 2048"]
    assert cov["obs: rounds 8"] and cov["lane: nblocks 5"]


def test_check_rows_are_few_fixed_and_at_the_ends_of_the_waves_of_lanes():
    for c in ds.CASES:
        rows = ds.check_rows(c.nprop, c.ndata)
        assert np.array_equal(rows, np.unique(rows)) and rows[0] == 0 and rows[-1] == c.nprop - 1
        if c.nprop * c.ndata <= ds.FULL_ROWS:
            assert rows.size == c.nprop
        else:
            assert rows.size <= ds.SUBSET_ROWS and rows.size * c.ndata <= ds.MAX_TERMS
            assert np.any(rows % 64 == 0) and np.any(rows % 64 == 63)
            last = (c.nprop - 1) // 64 * 64
            assert last == 0 or (last in rows and last - 1 in rows), "the start of the last wave of lanes"
        assert np.array_equal(rows, ds.check_rows(c.nprop, c.ndata))


@pytest.mark.parametrize("c", ds.CASES, ids=ds.case_id)
def test_the_reference_tells_the_tree_from_a_left_to_right_sum(c):
    """A condition on the inputs: on this case's data and rows the pairwise tree and the sequential sum differ in the last bits of at
    least one row in ten (cases of 17 observations or more; measured: 47 % of rows at 17 observations, 98 % at 20 001)."""
    D, X = ds.inputs(c)
    rows = ds.check_rows(c.nprop, c.ndata)
    want = ds.reg_reference(X[rows], D)
    assert want.shape == (rows.size,) and np.all(np.isfinite(want))
    np.testing.assert_allclose(want[:4], ds.sequential(ds.reg_terms(X[rows[:4]], D, ds.P0)), rtol=1e-9)      # (it is the sum)
    if c.ndata >= 17:
        differ, total = ds.vacuity(c)
        assert total >= (64 if c.nprop < 64 else rows.size)
        assert 10 * differ >= total, "%d of %d rows" % (differ, total)


BLOCKED = [c for c in ds.CASES if c.ndata >= 65][::3]


@pytest.mark.parametrize("c", BLOCKED, ids=ds.case_id)
def test_the_reference_tells_the_tree_from_one_cut_into_blocks_of_48(c):
    """... and from a tree over blocks that are no aligned power of two, what a wrong cut of the observations would compute."""
    differ, total = ds.vacuity(c, other=ds.blocked)
    assert differ >= 1, "%d of %d rows" % (differ, total)


def test_the_vacuity_yardsticks_are_what_they_say():
    rng = np.random.default_rng(3)
    T = rng.standard_normal((5, 200))
    seq = np.zeros(5)
    for j in range(200):
        seq = seq + T[:, j]
    np.testing.assert_array_equal(ds.sequential(T), seq)
    want = [recursive([recursive(list(T[r, j:j + 48])) for j in range(0, 200, 48)]) for r in range(5)]
    np.testing.assert_array_equal(ds.blocked(T), want)
    np.testing.assert_array_equal(ds.blocked(T, 64), pairwise(T))            # aligned power-of-two blocks: the same tree


def test_reference_follows_the_contract_on_non_finite_values():
    """-inf wins over a NaN or +inf tree sum only through the prior; inside the tree IEEE rules hold."""
    inf, nan = np.inf, np.nan
    T = np.array([[1.0, -inf, 2.0], [1.0, nan, 2.0], [inf, 1.0, -inf], [inf, 1.0, 2.0], [1.0, 2.0, 3.0]])
    term = lambda X, D: T
    got = ds.reference(term, None, np.zeros((5, 1)), None)
    np.testing.assert_array_equal(got, [-inf, nan, nan, inf, 6.0])
    pri = np.array([-inf, -inf, -inf, 0.5, -inf])
    np.testing.assert_array_equal(ds.reference(term, lambda X: pri, np.zeros((5, 1)), None), [-inf, -inf, -inf, inf, -inf])
    np.testing.assert_array_equal(ds.reference(term, lambda X: np.full(5, 0.5), np.zeros((5, 1)), None), [-inf, nan, nan, inf, 6.5])


def test_the_largest_reference_is_small_and_quick():
    """At most MAX_TERMS terms at once (160 MB), and seconds: measured 0.2 s for 16 rows of 600 000 terms."""
    terms = [(ds.check_rows(c.nprop, c.ndata).size * c.ndata, c) for c in ds.CASES]
    assert max(t for t, _ in terms) <= ds.MAX_TERMS
    _, c = max(terms)
    t0 = time.time()
    D, X = ds.inputs(c)
    ds.reg_reference(X[ds.check_rows(c.nprop, c.ndata)], D)
    assert time.time() - t0 < 10.0
