"""_native.SearchCall, the one route of the four search wrappers to their entry point, on a recording stand-in
for the library: the name and the engine of each family, the workspace rule (0 bytes asked for an empty shape, at
least 8 allocated, a large enough tensor reused) and where the bitmap and the engine go in the call.  CPU only."""
import pytest
import torch

from vectorragquantization_amd import _native as N


class FakeLib:
    def __init__(self, size=1000, rc=N.VRQ_OK):
        self.size, self.rc, self.calls = size, rc, []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return self.size if name.endswith("_workspace_size") else self.rc
        return fn


@pytest.fixture(autouse=True)
def no_stream(monkeypatch):
    monkeypatch.setattr(N, "stream_handle", lambda device=None: 77)


ALLOW = torch.zeros(4, dtype=torch.int64)
FAMILIES = [  # (K, allow, engine) -> name, engine value, bitmap argument
    ((10, None, None), "vrq_x", None, False), ((1025, None, None), "vrq_x_large", None, False),
    ((10, ALLOW, None), "vrq_x_filtered", None, True), ((5000, ALLOW, None), "vrq_x_filtered", None, True),
    ((10, None, "auto"), "vrq_x_batch", N.VRQ_LARGE_ENGINE_AUTO, True),
    ((5000, ALLOW, "mfma"), "vrq_x_batch", N.VRQ_LARGE_ENGINE_MFMA, True),
]


@pytest.mark.parametrize("case", FAMILIES, ids=[c[1] + str(i) for i, c in enumerate(FAMILIES)])
def test_name_engine_and_argument_order(case):
    (K, allow, engine), name, eng, bitmap = case
    call = N.SearchCall("vrq_x", K, 0, allow, engine)
    assert (call.name, call.engine, call.bitmap) == (name, eng, bitmap)
    assert N.SearchCall("vrq_x", K, 0, allow, engine, plain="vrq_x_dim").name == (name if name != "vrq_x" else "vrq_x_dim")
    lib, ws = FakeLib(), torch.zeros(16, dtype=torch.uint8)
    call(lib, (1, 2), (3, 4), allow, ws, "cpu")
    want = (1, 2) + ((N.ptr(allow),) if bitmap else ()) + (3, 4, N.ptr(ws), 16, 77) + (() if eng is None else (eng,))
    assert lib.calls == [(name, want)]
    with pytest.raises(N.VrqNativeError, match="label"):
        call(FakeLib(rc=N.VRQ_EWORKSPACE), (), (), allow, ws, "cpu", "label")


def test_workspace_rule():
    call = N.SearchCall("vrq_x", 2000)
    lib = FakeLib(size=1000)
    assert call.workspace_bytes(lib, 100, 128, 3, 2000) == 1000 and lib.calls == [("vrq_x_large_workspace_size", (100, 128, 3, 2000))]
    for empty in ((0, 128, 3, 2000), (100, 128, 0, 2000), (100, 128, 3, 0)):
        assert call.workspace_bytes(lib, *empty) == 0 and len(lib.calls) == 1       # the library is not asked
        assert call.workspace(lib, *empty, "cpu").numel() == 8
    assert call.workspace(FakeLib(size=3), 100, 128, 3, 2000, "cpu").numel() == 8
    ws = call.workspace(lib, 100, 128, 3, 2000, "cpu")
    assert ws.numel() == 1000 and ws.dtype == torch.uint8
    assert call.workspace(lib, 100, 128, 3, 2000, "cpu", ws) is ws
    assert call.workspace(lib, 100, 128, 3, 2000, "cpu", ws[:999]).numel() == 1000


def test_refusals_name_the_caller():
    with pytest.raises(N.VrqNativeError, match=r"here: K = 9000.*8192"):
        N.SearchCall("vrq_x", 9000, what="here")
    with pytest.raises(N.VrqNativeError, match="vrq_x: flags 4 with a row filter"):
        N.SearchCall("vrq_x", 10, N.VRQ_SEARCH_SCAN_VALU, ALLOW)
    with pytest.raises(N.VrqNativeError, match="flags 2 with engine='valu'"):
        N.SearchCall("vrq_x", 10, N.VRQ_SEARCH_SHARD, ALLOW, "valu")
