"""The Python side of the per-query filters, without a launch: filters.row_bitmaps / ids_bitmaps against NumPy's
packbits per set, the checker's refusals, the wrappers' routing read from the SearchCall object alone, and
allowed_ids_per_query being turned into sets and a query_set."""
import numpy as np
import pytest
import torch

from vectorragquantization_amd import _native as N
from vectorragquantization_amd import filters as F

SIZES = (1, 63, 64, 65, 12_325)


def packed(mask):
    """bool[n] -> int64 words, NumPy only."""
    n = mask.shape[0]
    by = np.zeros(((n + 63) // 64) * 8, np.uint8)
    p = np.packbits(mask, bitorder="little")
    by[:p.shape[0]] = p
    return by.view(np.int64)


@pytest.mark.parametrize("n", SIZES)
def test_row_bitmaps_against_packbits(n):
    rng = np.random.default_rng(n)
    masks = np.stack([rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool), np.arange(n) == n - 1,
                      rng.random(n) < 0.02])
    got = F.row_bitmaps(torch.from_numpy(masks))
    assert got.dtype == torch.int64 and tuple(got.shape) == (5, F.words(n)) and got.is_contiguous()
    for s in range(5):
        assert np.array_equal(got[s].numpy(), packed(masks[s]))
        assert np.array_equal(got[s].numpy(), F.row_bitmap(torch.from_numpy(masks[s])).numpy())
    with pytest.raises(N.VrqNativeError, match="S, n"):
        F.row_bitmaps(torch.from_numpy(masks[0]))


@pytest.mark.parametrize("n", SIZES)
def test_ids_bitmaps_against_packbits(n):
    rng = np.random.default_rng(100 + n)
    ids = rng.permutation(np.arange(1000, 1000 + n)).astype(np.int64)
    if n > 2:
        ids[2] = ids[0]   # a duplicated id: both rows
    id_map = torch.from_numpy(ids)
    a = ids[rng.random(n) < 0.5].tolist()
    entries = [a, None, [], list(reversed(a)), [ids[0], 5, 7], torch.tensor([int(ids[0])]), None, [5, 7],
               set(a)]
    allow, qs = F.ids_bitmaps(id_map, entries)
    assert allow.dtype == torch.int64 and allow.shape[1] == F.words(n) and qs.dtype == torch.int32
    qs = qs.tolist()
    assert len(qs) == len(entries) and qs[1] == qs[6] == -1
    assert qs[0] == qs[3] == qs[8]                     # equal collections share a set, whatever their order or type
    assert allow.shape[0] == len({s for s in qs if s >= 0}) == max(qs) + 1
    for e, s in zip(entries, qs):
        if e is None:
            continue
        want = np.isin(ids, np.array([int(i) for i in (e.tolist() if isinstance(e, torch.Tensor) else e)], np.int64))
        assert np.array_equal(allow[s].numpy(), packed(want)), e
        assert np.array_equal(allow[s].numpy(), F.ids_bitmap(id_map, list(e) if not isinstance(e, torch.Tensor) else e).numpy())
    # an empty collection and one of unknown ids: all-zero bitmaps (they may share one: both are no row)
    assert not allow[qs[2]].any() and not allow[qs[7]].any()


def test_ids_bitmaps_without_a_collection_still_has_one_set():
    allow, qs = F.ids_bitmaps(torch.arange(70), [None, None, None])
    assert tuple(allow.shape) == (1, 2) and not allow.any() and qs.tolist() == [-1, -1, -1]


def test_checked_sets_refusals():
    n, nq = 130, 4
    allow = torch.zeros((3, F.words(n)), dtype=torch.int64)
    qs = torch.tensor([0, 2, -1, 5], dtype=torch.int32)
    a, q = F.checked_sets(allow, qs, n, nq, "cpu")
    assert a is allow and q.dtype == torch.int32 and q.tolist() == [0, 2, -1, 5]
    # wider rows are fine (bitmaps sized for capacity), also as a strided view; int64 ids are converted
    wide = torch.zeros((3, F.words(n) + 3), dtype=torch.int64)
    a, q = F.checked_sets(wide, qs.to(torch.int64), n, nq, "cpu")
    assert a is wide and q.dtype == torch.int32
    view = wide[:, :F.words(n)]
    a, _ = F.checked_sets(view, qs, n, nq, "cpu")
    assert a.stride(0) == F.words(n) + 3 and a.stride(1) == 1 and a.data_ptr() == wide.data_ptr()
    a, _ = F.checked_sets(wide[:, ::2], qs, 64, nq, "cpu")          # not unit stride: a contiguous copy
    assert a.is_contiguous()
    # set_words is the row stride; one set may carry any stride along its size-1 dimension and is as wide as its row
    assert N.set_words_of(wide) == N.set_words_of(view) == F.words(n) + 3 and N.set_words_of(allow) == F.words(n)
    lone = torch.zeros(8, dtype=torch.int64).as_strided((1, F.words(n)), (1, 1))
    a, _ = F.checked_sets(lone, qs, n, nq, "cpu")
    assert N.set_words_of(a) == F.words(n) >= F.words(n)
    bad = [
        (allow.to(torch.int32), qs),                                # dtype
        (allow[0], qs),                                             # 1-D
        (allow[:, :F.words(n) - 1], qs),                            # too few words
        (allow[:0], qs),                                            # no set
        (allow.numpy(), qs),                                        # not a tensor
        (allow, qs[:3]),                                            # query_set of another length
        (allow, qs.to(torch.float32)),                              # not integers
        (allow, qs.reshape(2, 2)),                                  # not 1-D
        (allow, [0, 2, -1, 5]),                                     # not a tensor
    ]
    for a, q in bad:
        with pytest.raises(N.VrqNativeError):
            F.checked_sets(a, q, n, nq, "cpu")
    with pytest.raises(N.VrqNativeError, match="is on"):
        F.checked_sets(allow, qs, n, nq, "meta")
    # checked_filter: the 1-D path is filters.checked, untouched
    one = torch.zeros(F.words(n), dtype=torch.int64)
    assert F.checked_filter(None, None, n, nq, "cpu") == (None, None)
    a, q = F.checked_filter(one, None, n, nq, "cpu")
    assert a.data_ptr() == one.data_ptr() and q is None
    with pytest.raises(N.VrqNativeError):
        F.checked_filter(allow, None, n, nq, "cpu")                 # 2-D without query_set


# ---- routing, from the SearchCall object alone ----
BASES = ("vrq_search3", "vrq_search2", "vrq_hamming_topk")


def test_search_call_names_the_perquery_call():
    one = torch.zeros(4, dtype=torch.int64)
    sets = torch.zeros((3, 4), dtype=torch.int64)
    qs = torch.zeros(2, dtype=torch.int32)
    lib = N.load()
    for base in BASES:
        for K in (10, 5000, 8192):
            # 1-D allow without query_set: exactly the route it was
            assert N.SearchCall(base, K, 0, one).name == base + "_filtered"
            assert N.SearchCall(base, K, 0, one).engine is None and not N.SearchCall(base, K, 0, one).perquery
            assert N.SearchCall(base, K, 0, one, "mfma").name == base + "_batch"
            # 2-D allow with query_set: the per-query call; engine=None means AUTO
            c = N.SearchCall(base, K, 0, sets, None, query_set=qs)
            assert c.name == base + "_perquery" and c.perquery and c.bitmap and c.engine == N.VRQ_LARGE_ENGINE_AUTO
            for e, v in (("auto", 0), ("valu", 1), ("mfma", 2)):
                c = N.SearchCall(base, K, 0, sets, e, query_set=qs)
                assert c.name == base + "_perquery" and c.engine == v
            # its workspace is the batch call's: there is no *_perquery_workspace_size
            width = 128 if base == "vrq_hamming_topk" else 1024
            assert c.workspace_bytes(lib, 20000, width, 2, K) == \
                getattr(lib, base + "_batch_workspace_size")(20000, width, 2, K) > 0
            assert c.workspace_bytes(lib, 0, width, 2, K) == 0
        with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
            N.SearchCall(base, 9000, 0, sets, None, query_set=qs)
        for flag in (N.VRQ_SEARCH_SHARD, N.VRQ_SEARCH_SCAN_MFMA, N.VRQ_SEARCH_SCAN_VALU):
            with pytest.raises(N.VrqNativeError, match="flags"):
                N.SearchCall(base, 10, flag, sets, None, query_set=qs)
        N.SearchCall(base, 10, N.VRQ_SEARCH_PHASE1_ONLY, sets, None, query_set=qs)
        with pytest.raises(N.VrqNativeError, match="engine"):
            N.SearchCall(base, 10, 0, sets, "fast", query_set=qs)
        with pytest.raises(N.VrqNativeError, match="query_set"):
            N.SearchCall(base, 10, 0, sets)                          # 2-D allow without query_set
        with pytest.raises(N.VrqNativeError, match="allow"):
            N.SearchCall(base, 10, 0, None, query_set=qs)            # query_set without allow


def test_search3_route_and_the_wrappers_raise_before_any_launch():
    from vectorragquantization_amd import quant as Q
    from vectorragquantization_amd.enhanced import search3, search3_route
    from vectorragquantization_amd.index import BinaryIndexIDMap2
    n, d, nq = 9000, 256, 2
    w = F.words(n)
    sets = torch.zeros((3, w), dtype=torch.int64)
    qs = torch.tensor([0, -1], dtype=torch.int32)
    assert search3_route(10, 0, sets, None, qs).name == "vrq_search3_perquery"
    assert search3_route(10, N.VRQ_SEARCH_PHASE1_ONLY, sets, "valu", qs).engine == N.VRQ_LARGE_ENGINE_VALU
    assert search3_route(10, 0, sets[0]).name == "vrq_search3_filtered"
    with pytest.raises(N.VrqNativeError, match="flags"):
        search3_route(10, N.VRQ_SEARCH_SHARD, sets, None, qs)
    codes = torch.zeros((n, d // 8), dtype=torch.uint8)
    qf, qb = torch.zeros((nq, d)), torch.zeros((nq, d // 8), dtype=torch.uint8)
    x8, norms = torch.zeros((n, d), dtype=torch.int8), torch.zeros(n, dtype=torch.float64)
    # K past the limit, the sharded mode and the scan flags
    with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
        Q.search2("sbin", codes, codes, qf, qb, 900, 10, allow=sets, query_set=qs)
    with pytest.raises(N.VrqNativeError, match="flags"):
        Q.search2("sbin", codes, codes, qf, qb, 10, 10, flags=N.VRQ_SEARCH_SCAN_VALU, allow=sets, query_set=qs)
    with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
        Q.vectordb_search("bin16", codes, None, None, qb, 900, 10, allow=sets, query_set=qs)
    with pytest.raises(N.VrqNativeError, match="flags"):
        search3(codes, x8, norms, qf, qb, 10, 100, 30, flags=N.VRQ_SEARCH_SHARD, allow=sets, query_set=qs)
    # a 2-D allow without query_set, a query_set of the wrong length, too few words
    with pytest.raises(N.VrqNativeError, match="query_set"):
        Q.search2("sbin", codes, codes, qf, qb, 10, 10, allow=sets)
    with pytest.raises(N.VrqNativeError, match="query_set"):
        Q.vectordb_search("bin16", codes, None, None, qb, 10, 10, allow=sets, query_set=qs[:1])
    with pytest.raises(N.VrqNativeError, match="allow"):
        Q.search2("sbin", codes, codes, qf, qb, 10, 10, allow=sets[:, :w - 1], query_set=qs)
    with pytest.raises(N.VrqNativeError, match="allow"):
        search3(codes, x8, norms, qf, qb, 10, 100, 30, allow=sets.to(torch.int32), query_set=qs)
    ix = BinaryIndexIDMap2(d, "cpu")
    ix.add_with_ids(codes.numpy(), np.arange(n, dtype=np.int64))
    with pytest.raises(N.VrqNativeError, match="query_set"):
        ix.search_device(qb, 10, allow=sets)
    with pytest.raises(N.VrqNativeError, match="query_set"):
        ix.search_device(qb, 10, allow=sets, query_set=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
        ix.search_device(qb, 9000, allow=sets, query_set=qs)


def test_class_filter_turns_entries_into_sets_and_query_set():
    id_map = torch.arange(500, 700, dtype=torch.int64)
    assert F.class_filter(id_map, None, None, 3) == (None, None)
    a, q = F.class_filter(id_map, [500, 501], None, 3)
    assert q is None and a.dim() == 1 and np.array_equal(a.numpy(), packed(np.arange(200) < 2))
    entries = [None, [500, 650], [], [650, 500], (1, 2, 3), None]
    a, q = F.class_filter(id_map, None, entries, 6)
    assert q.dtype == torch.int32 and q.tolist() == [-1, 0, 1, 0, 2, -1] and tuple(a.shape) == (3, F.words(200))
    assert np.array_equal(a[0].numpy(), packed(np.isin(np.arange(500, 700), [500, 650])))
    assert not a[1].any() and not a[2].any()                        # empty, and unknown ids: nothing is found
    assert N.SearchCall("vrq_search2", 100, 0, a, None, query_set=q).name == "vrq_search2_perquery"
    with pytest.raises(N.VrqNativeError, match="exclusive"):
        F.class_filter(id_map, [500], entries, 6)
    with pytest.raises(N.VrqNativeError, match="6 entries for 5"):
        F.class_filter(id_map, None, entries, 5)
