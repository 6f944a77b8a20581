"""CPU test of tests/pairwise_model.py: the restated plan of the encoder's pairwise float32 sum, replayed
in np.float32, IS NumPy's sum -- at the dims whose plans differ in shape and at every multiple of 8 up to
the encoder's largest dim.  tests/test_gpu_encode_dims.py relies on it twice: ``plan_shape`` decides
whether its dim list reaches every path of the kernel, and the wrong sums of the model (sequential, leaf
sums folded left to right) are what its near-mean rows have to tell from the true mean."""
import numpy as np
import pytest

import pairwise_model as P

# dim -> (leaves, bal_levels, distinct leaf lengths)
TABLE = {
    8: (1, 0, {8}), 128: (1, 0, {128}),
    136: (2, 1, {64, 72}),
    264: (3, -1, {64, 72, 128}),
    384: (4, 2, {96}), 512: (4, 2, {128}),
    768: (8, 3, {96}), 1000: (8, 3, {120, 128}), 1024: (8, 3, {128}),
    1032: (9, -1, {64, 72, 128}),
    1536: (16, -1, {96}), 2048: (16, -1, {128}),
    2056: (17, -1, {64, 72, 128}),
    4096: (32, -1, {128}), 8192: (64, -1, {128}),
}


def _rows(rng, n, d):
    """Rows of different scales and offsets: means away from 0, partial sums that round at every step."""
    X = rng.standard_normal((n, d)) * rng.uniform(0.01, 2.0, (n, 1)) + rng.uniform(-1.0, 1.0, (n, 1))
    return X.astype(np.float32)


def _np_sums(X):
    return np.array([np.sum(x) for x in X], np.float32)       # one contiguous row at a time, as the oracle


@pytest.mark.parametrize("d", sorted(TABLE))
def test_plan_shape_and_replay_at_the_table_dims(d):
    nl, bal, lens = P.plan_shape(d)
    assert (nl, bal, set(lens)) == TABLE[d]
    assert sum(lens) == d and len(lens) == nl
    p = P.plan(d)
    assert p.start == list(np.cumsum([0] + list(lens[:-1])))
    assert p.ops.count(-1) == nl - 1 and sorted(o for o in p.ops if o >= 0) == list(range(nl))
    X = _rows(np.random.default_rng(d), 64, d)
    got, ref = P.replay(X), _np_sums(X)
    assert got.dtype == np.float32 and np.array_equal(got, ref)
    for x in X[:8]:                                            # np.mean itself, through the last division
        assert P.mean_of_sum(P.replay(x), d)[0] == np.mean(x)
    # the stack fold computes the balanced trees too: the butterfly is a shortcut, not another sum
    if bal >= 0:
        assert np.array_equal(P._fold_stack(P.leaf_sums(X), p), ref)
    S, steps = P.trace(X[0])
    assert np.array_equal(S, P.leaf_sums(X[:1])[0]) and len(steps) == nl - 1
    assert (steps[-1] if nl > 1 else S[0]) == ref[0]


def test_replay_equals_numpy_at_every_multiple_of_8():
    rng = np.random.default_rng(8192)
    for d in range(8, P.MAX_DIM + 1, 8):
        X = _rows(rng, 3, d)
        assert np.array_equal(P.replay(X), _np_sums(X)), d
        assert P.plan(d).nleaves <= P.MAX_LEAVES


def test_dims_that_are_no_multiple_of_8_have_leaf_tails():
    """The encoder takes multiples of 8 only; the model still restates the leaf's sequential tail."""
    rng = np.random.default_rng(5)
    for d in (1, 7, 9, 127, 129, 1001, 2055):
        X = _rows(rng, 16, d)
        assert np.array_equal(P.replay(X), _np_sums(X)), d


def test_the_wrong_sums_are_wrong():
    """The two mistakes the GPU test's inputs are built against differ from NumPy's sum on random rows
    (so a test input CAN tell them apart), and agree with it where they must: one leaf / two leaves."""
    X = _rows(np.random.default_rng(1), 200, 2048)
    ref = _np_sums(X)
    assert (P.sum_sequential(X) != ref).mean() > 0.5
    assert (P.sum_leaves_left_fold(X) != ref).mean() > 0.2
    Y = _rows(np.random.default_rng(2), 50, 136)
    assert np.array_equal(P.sum_leaves_left_fold(Y), _np_sums(Y))


def test_shape_classes_of_the_known_dims():
    assert P.shape_classes(16) == {"one leaf"}
    assert P.shape_classes(136) == {"balanced, unequal leaves"}
    assert P.shape_classes(1000) == {"balanced, unequal leaves"}
    assert P.shape_classes(264) == {"stack fold, one batch"}
    assert P.shape_classes(1024) == {"balanced, equal leaves"}
    assert P.shape_classes(1032) == {"9 leaves"} and P.shape_classes(2056) == {"17 leaves"}
    assert P.shape_classes(1536) == P.shape_classes(2048) == {"16 leaves"}
    assert P.shape_classes(4096) == {"32 leaves"} and P.shape_classes(8192) == {"64 leaves"}
    # every dim of the GPU suite before tests/test_gpu_encode_dims.py: no stack fold, no second batch
    old = set().union(*(P.shape_classes(d) for d in (1024, 384, 768, 1000, 128, 8, 256)))
    assert old == {"one leaf", "balanced, unequal leaves", "balanced, equal leaves"}
