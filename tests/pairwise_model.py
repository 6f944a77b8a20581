"""Pure-Python restatement of the encoder's pairwise-sum plan (encode.hip: ``pw_build``, ``pw_classify``,
``pairwise_sum_f32``) and a replay of it in ``np.float32`` arithmetic.  Test infrastructure only, no
product code.

NumPy sums a contiguous float32 row pairwise: rows of at most 128 elements are one leaf (8 strided
accumulators, the fixed tree ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then a sequential tail), longer rows
split at ``n // 2`` rounded down to a multiple of 8 and add the two halves.  The leaf / tree structure
depends on n alone; the host builds it as a plan and the kernel replays it:

  plan(dim)        the leaves (start, length) in order and the postfix program that folds them
                   (>= 0: push that leaf's sum, -1: add the top two), plus ``bal_levels``: L when the
                   program is the balanced tree over 2^L <= 8 leaves (the kernel then folds with a lane
                   butterfly instead of the LDS stack), else -1
  plan_shape(dim)  (nleaves, bal_levels, leaf lengths in order): what a dim exercises
  shape_classes(dim)  the names of the plan shapes a dim list has to cover between its members
  replay(X)        the kernel's sum of every row of X, float32: leaves in batches of 8 (lane 8g + j
                   holds column j of leaf b + g), then the butterfly or the stack

``replay`` equals ``np.sum`` on float32 rows (tests/test_pairwise_model.py).  The other sums here are the
mistakes a kernel could make, used to show that a test's inputs can tell them from the true mean:
``sum_sequential`` (one accumulator, left to right) and ``sum_leaves_left_fold`` (the right leaf sums,
folded left to right instead of in the recursion's order).  ``trace(x)`` lists every leaf sum and every
fold step of one row, to name the step at which another implementation's sum departs.
"""
import numpy as np

LEAF_MAX = 128      # NumPy's PW_BLOCKSIZE
BATCH = 8           # leaves per pass of the kernel's batch loop (8 lanes per leaf, 64 lanes)
MAX_LEAVES = 128    # encode.hip
MAX_DIM = 8192


# ------------------------------------------------------------------------------------------------
# pw_build / pw_classify
class Plan:
    def __init__(self, dim):
        self.dim = dim
        self.start, self.len, self.ops = [], [], []
        _build(0, dim, self)
        self.nleaves = len(self.start)
        self.bal_levels = _classify(self)


def _build(s, n, p):
    if n <= LEAF_MAX:
        p.ops.append(len(p.start))
        p.start.append(s)
        p.len.append(n)
        return
    n2 = n // 2
    n2 -= n2 % 8
    _build(s, n2, p)
    _build(s + n2, n - n2, p)
    p.ops.append(-1)


def _balanced(first, L, ops):
    """postfix of the balanced tree over leaves [first, first + 2^L): left, right, add"""
    if L == 0:
        ops.append(first)
        return
    _balanced(first, L - 1, ops)
    _balanced(first + (1 << (L - 1)), L - 1, ops)
    ops.append(-1)


def _classify(p):
    bal = -1
    for L in range(4):
        if p.nleaves != 1 << L:
            continue
        ops = []
        _balanced(0, L, ops)
        if ops == p.ops:
            bal = L
    return bal


_plans = {}


def plan(dim):
    if dim not in _plans:
        _plans[dim] = Plan(dim)
    return _plans[dim]


def plan_shape(dim):
    """(nleaves, bal_levels, leaf_lengths): the leaf count, the balanced-tree depth (-1: the stack fold)
    and the leaf lengths in order."""
    p = plan(dim)
    return p.nleaves, p.bal_levels, tuple(p.len)


def shape_classes(dim):
    """The plan shapes of the encoder that dim belongs to (a set of names).  A dim list covers the
    encoder's paths when the union over its members is ``ALL_SHAPE_CLASSES``."""
    nl, bal, lens = plan_shape(dim)
    out = set()
    if nl == 1:
        out.add("one leaf")
    if bal >= 1 and len(set(lens)) > 1:
        out.add("balanced, unequal leaves")
    if bal >= 1 and len(set(lens)) == 1:
        out.add("balanced, equal leaves")
    if bal < 0 and nl <= BATCH:
        out.add("stack fold, one batch")
    if nl in (9, 16, 17, 32, 64):
        out.add(f"{nl} leaves")
    return out


ALL_SHAPE_CLASSES = {"one leaf", "balanced, unequal leaves", "balanced, equal leaves", "stack fold, one batch",
                     "9 leaves", "16 leaves", "17 leaves", "32 leaves", "64 leaves"}


# ------------------------------------------------------------------------------------------------
# the replay, float32 throughout (every a + b below is one float32 addition, rounded once)
def _rows(X):
    X = np.asarray(X)
    assert X.dtype == np.float32
    return X.reshape(-1, X.shape[-1])


def leaf_sums(X):
    """f32[rows, nleaves]: each leaf's sum as lanes 8g..8g+7 of the kernel compute it."""
    X = _rows(X)
    p = plan(X.shape[1])
    out = np.zeros((X.shape[0], p.nleaves), np.float32)
    for m in sorted(set(p.len)):                                  # the leaves of one length together
        which = [i for i in range(p.nleaves) if p.len[i] == m]
        idx = np.asarray([p.start[i] for i in which])[:, None] + np.arange(m)[None, :]
        L = X[:, idx]                                             # [rows, leaves, m]
        m8 = m - m % 8
        if m >= 8:
            r = L[:, :, 0:8].copy()                               # lane j: column j, sequentially
            for i in range(8, m8, 8):
                r = r + L[:, :, i:i + 8]
            t = r[:, :, 0::2] + r[:, :, 1::2]                     # xor 1: r0+r1, r2+r3, r4+r5, r6+r7
            t = t[:, :, 0::2] + t[:, :, 1::2]                     # xor 2
            res = t[:, :, 0] + t[:, :, 1]                         # xor 4
            i0 = m8
        else:
            res = np.zeros(L.shape[:2], np.float32)
            i0 = 0
        for i in range(i0, m):                                    # the tail, by the leaf's first lane
            res = res + L[:, :, i]
        assert res.dtype == np.float32
        out[:, which] = res
    return out


def _fold_stack(S, p, steps=None):
    st = []
    for op in p.ops:
        if op >= 0:
            st.append(S[:, op])
        else:
            rgt = st.pop()
            lft = st.pop()
            st.append(lft + rgt)
            if steps is not None:
                steps.append(st[-1])
    assert len(st) == 1
    return st[0]


def _fold_butterfly(S, p):
    """Leaf g in lane group g of 8 (0 where there is no leaf), xor 8, 16, 32 as far as bal_levels."""
    a = np.zeros((S.shape[0], BATCH), np.float32)
    a[:, :p.nleaves] = S
    for lvl in range(p.bal_levels):
        a = a + a[:, np.arange(BATCH) ^ (1 << lvl)]
    return a[:, 0]


def replay(X):
    """The kernel's pairwise sum of every row, f32[rows]."""
    X = _rows(X)
    p = plan(X.shape[1])
    S = leaf_sums(X)
    out = _fold_butterfly(S, p) if p.bal_levels >= 0 else _fold_stack(S, p)
    assert out.dtype == np.float32
    return out


def mean_of_sum(s, dim):
    """np.mean's last step: np.float32(sum) / n, one rounding to float32."""
    return (np.asarray(s, np.float32).astype(np.float64) / float(dim)).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# the sums a wrong kernel would compute
def sum_sequential(X):
    """One float32 accumulator over the row, left to right."""
    X = _rows(X)
    s = np.zeros(X.shape[0], np.float32)
    for i in range(X.shape[1]):
        s = s + X[:, i]
    return s


def sum_leaves_left_fold(X):
    """The true leaf sums, folded ((L0 + L1) + L2) + ... instead of in the recursion's order."""
    S = leaf_sums(X)
    s = S[:, 0].copy()
    for i in range(1, S.shape[1]):
        s = s + S[:, i]
    return s


def trace(x):
    """One row -> (leaf sums f32[nleaves], fold results f32[number of -1 ops] in program order)."""
    X = _rows(x)
    assert X.shape[0] == 1
    p = plan(X.shape[1])
    S = leaf_sums(X)
    steps = []
    _fold_stack(S, p, steps)
    return S[0], np.asarray([v[0] for v in steps], np.float32)
