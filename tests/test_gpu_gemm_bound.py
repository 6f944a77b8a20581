"""K5 (gemm_topk.hip: vrq_gemm_topk / vrq_flat_ip_topk) is exact by a proof, not by an exhaustive scan:
a row whose matrix-core value u falls below thr = U - 2 Delta is never rescored.  These tests pin the
proof's ingredients down on the GPU, each against a plain float64 restatement (tests/gemm_bound_model.py):

  1. the prep kernel: pieces, Delta, alpha, beta of every mode, bit for bit / to 1e-12
  2. the sample pass: every lane maximum dv against a float64 GEMM of the checked pieces
  3. the select kernel: thr against a sort of the kernel's own dv and Delta
  4. soundness on inputs that attain the bound: with Delta 10 % smaller, min for max of the one-sided
     sums, or thr = U - Delta, a true top-k row is lost (tests/test_gemm_bound_model.py proves that of
     the fixtures on the CPU)
  5. query scale: 2^+-60 and float32-subnormal queries
  6. the retry pass of the binary and int8-cosine modes at the smallest n whose chunks can overflow

Every helper takes ``lib=`` (another build of the library), default the in-tree libvrq.so.
"""
import numpy as np
import pytest
import torch

import gemm_bound_model as M
from oracle import oracle_np as O
from test_gpu_lists import _bits, _ph2_perm

pytestmark = pytest.mark.gpu

D = 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


def _t(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)   # (the shared fixtures are read-only)


def _mode_id(mode):
    from vectorragquantization_amd import _native as N
    return {"binary": N.VRQ_GEMM_BINARY, "int8_cosine": N.VRQ_GEMM_INT8_COSINE, "float_ip": N.VRQ_GEMM_FLOAT_IP}[mode]


class Corpus:
    """Device operands of one mode: codes (binary), x8 + norms (int8_cosine), xf + x8 + 1/scale + bounds
    (float_ip, through vrq_flat_ip_prepare)."""

    def __init__(self, mode, dev, codes=None, x8=None, xf=None):
        from vectorragquantization_amd.flat import flat_ip_prepare
        from vectorragquantization_amd.quant import int8_row_norms
        as_t = lambda a: a if a is None or torch.is_tensor(a) else _t(a, dev)
        self.mode, self.dev = mode, dev
        self.codes, self.x8, self.xf, self.norms, self.bounds = as_t(codes), as_t(x8), as_t(xf), None, None
        if mode == "int8_cosine":
            self.norms = int8_row_norms(self.x8)
        elif mode == "float_ip":
            self.bounds = torch.zeros(2, dtype=torch.float64, device=dev)
            self.x8, self.norms = flat_ip_prepare(self.xf, self.bounds)
        self.n = (self.codes if mode == "binary" else self.x8).shape[0]


class Layout:
    def __init__(self, mode, n, nq, k, lib=None):
        from vectorragquantization_amd import _native as N
        lib = lib or N.load()
        plan, lay, prep = np.zeros(8, np.int64), np.zeros(8, np.int64), np.zeros(4, np.int64)
        args = (_mode_id(mode), n, D, nq, k)
        N.check(lib.vrq_gemm_topk_plan(*args, plan.ctypes.data), "plan")
        N.check(lib.vrq_gemm_topk_layout(*args, lay.ctypes.data), "layout")
        N.check(lib.vrq_gemm_topk_prep_layout(*args, prep.ctypes.data), "prep layout")
        self.nq, self.n = nq, n
        self.chunk_rows, self.nchunks, self.capc, self.nqb, self.nsc, _, self.bytes, self.gqb = (int(x) for x in plan)
        self.nq_pad, self.off_thr, self.off_cnt, self.off_cand, self.off_dv, self.scols, self.sstride, self.scr = (
            int(x) for x in lay)
        self.off_delta, self.off_alpha, self.off_beta, self.off_flag = (int(x) for x in prep)

    def _f64(self, ws, off):
        return ws[off:off + 8 * self.nq_pad].view(torch.float64).cpu().numpy()

    def qa(self, ws):
        return ws[:self.nq_pad * D].view(torch.int8).view(self.nq_pad, D)

    def delta(self, ws):
        return self._f64(ws, self.off_delta)

    def alpha(self, ws):
        return self._f64(ws, self.off_alpha)

    def beta(self, ws):
        return self._f64(ws, self.off_beta)

    def thr(self, ws):
        return ws[self.off_thr:self.off_thr + 4 * self.nq_pad].view(torch.float32).cpu().numpy()

    def dv(self, ws):
        return ws[self.off_dv:self.off_dv + 4 * self.nq * self.scols].view(torch.float32).view(self.nq, self.scols)

    def cnt(self, ws):
        return ws[self.off_cnt:self.off_cnt + 4 * self.nq * self.nchunks].view(torch.int32).view(self.nq, self.nchunks)


def _call(c, qf, k, flags=0, ws=None, lib=None):
    """One vrq_gemm_topk / vrq_flat_ip_topk call -> (count, rows, scores) as NumPy, and the workspace."""
    from vectorragquantization_amd import _native as N
    lib = lib or N.load()
    dev = c.dev
    q_t = qf if torch.is_tensor(qf) else _t(np.asarray(qf, np.float32), dev)
    nq = q_t.shape[0]
    need = lib.vrq_gemm_topk_workspace_size(_mode_id(c.mode), c.n, D, nq, k)
    assert need > 0
    if ws is None:
        ws = torch.zeros((need,), dtype=torch.uint8, device=dev)
    assert ws.numel() >= need
    cnt = torch.full((nq,), -2, dtype=torch.int32, device=dev)
    rows = torch.full((nq, k), -2, dtype=torch.int64, device=dev)
    sc = torch.empty((nq, k), dtype=torch.float64, device=dev)
    out = (N.ptr(q_t), nq, k, flags, N.ptr(cnt), N.ptr(rows), N.ptr(sc), N.ptr(ws), ws.numel(), N.stream_handle(dev))
    if c.mode == "float_ip":
        N.check(lib.vrq_flat_ip_topk(N.ptr(c.xf), N.ptr(c.x8), N.ptr(c.norms), N.ptr(c.bounds), c.n, D, 0, *out),
                "vrq_flat_ip_topk")
    else:
        N.check(lib.vrq_gemm_topk(_mode_id(c.mode), N.ptr(c.codes), N.ptr(c.x8), N.ptr(c.norms), c.n, D, 0, *out),
                "vrq_gemm_topk")
    torch.cuda.synchronize()
    return (cnt.cpu().numpy(), rows.cpu().numpy(), sc.cpu().numpy()), ws


def _stage():
    from vectorragquantization_amd import _native as N
    return N.VRQ_GEMM_STAGE_SAMPLE, N.VRQ_GEMM_STAGE_MAIN, N.VRQ_GEMM_NO_FALLBACK


def _pieces(lay, ws, mode):
    """The int8 pieces of the real queries in natural dim order, int8 device tensor [nq, 1024]."""
    a = lay.qa(ws)[:lay.nq]
    return a[:, torch.from_numpy(_ph2_perm()).to(a.device)] if mode == "binary" else a


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def _check_oracle(c, qf, k, res, codes=None, x8=None, F=None):
    """Rows, order and scores of the oracle (oracle.exhaustive_scores / exhaustive_topk, as
    test_gpu_gemm._check).  float_ip: the oracle's float64 dot and the GPU's may round differently to
    float32, so its scores are held to one float32 ulp (test_gpu_flat), the rows exactly."""
    cnt, rows, sc = res
    qf = np.asarray(qf, np.float32)
    S = O.flat_ip_scores(F, qf) if c.mode == "float_ip" else O.exhaustive_scores(c.mode, qf, codes=codes, x8=x8)
    ref = O.exhaustive_topk(S, k)
    m = min(k, S.shape[1])
    for q in range(qf.shape[0]):
        assert cnt[q] == m, (c.mode, q, cnt[q])
        assert np.array_equal(rows[q, :m], ref[q]), (c.mode, q, rows[q, :m], ref[q])
        if c.mode == "float_ip":
            assert np.all(np.abs(sc[q, :m] - S[q, ref[q]]) <= _ulp(S[q, ref[q]])), (c.mode, q)
        else:
            assert np.array_equal(sc[q, :m], S[q, ref[q]]), (c.mode, q)
        assert np.all(rows[q, m:] == -1)


# ------------------------------------------------------------------------------------------------
# 1. prep kernel
def _prep_queries():
    """257 queries (two query blocks, 255 padding queries) -> (qf f32[257, 1024], names of the special ones)."""
    rng = np.random.default_rng(101)
    qf = rng.standard_normal((257, D)).astype(np.float32)
    special = {}

    def put(name, v):
        special[name] = 200 + len(special)
        qf[special[name]] = v

    for name in ("binary_sym", "binary_asym", "int8_cosine", "float_ip"):
        for j, q in enumerate(M.fixture(name)["qf"]):
            put(f"{name}{j}", q)
    half = np.array([0.5, 1.5, 2.5, -0.5], np.float32)[np.arange(D) % 4]   # rint is half-to-even: 0, 2, 2, -0
    half[77] = 127.0
    put("half", half)
    put("half_neg", -half)
    spike = np.zeros(D, np.float32)
    spike[1023] = -3.25
    put("spike", spike)
    put("zero", np.zeros(D, np.float32))
    put("big", qf[0] * np.float32(2.0 ** 60))
    put("small", qf[0] * np.float32(2.0 ** -60))
    qf[256] = qf[1] * np.float32(2.0 ** -60)       # the only real query of the second block
    return qf, special


@pytest.mark.parametrize("mode", M.MODES)
def test_prep_kernel_vs_float64(dev, mode):
    SAMPLE, _, _ = _stage()
    rng = np.random.default_rng(102)
    qf, special = _prep_queries()
    n, k = 96, 10
    if mode == "binary":
        c = Corpus(mode, dev, codes=rng.integers(0, 256, (n, 128), dtype=np.uint8))
    elif mode == "int8_cosine":
        c = Corpus(mode, dev, x8=rng.integers(-127, 128, (n, D)).astype(np.int8))
    else:
        xf = rng.standard_normal((n, D)).astype(np.float32)
        xf[3] *= 25.0
        c = Corpus(mode, dev, xf=xf)
    lay = Layout(mode, n, qf.shape[0], k)
    assert (lay.nq_pad, lay.nqb) == (512, 2)
    _, ws = _call(c, qf, k, SAMPLE)
    bounds = c.bounds.cpu().numpy() if mode == "float_ip" else None
    ref = M.prep_reference(mode, qf, bounds)
    # the reference itself on the inputs whose pieces are known in closed form
    h = ref["a"][special["half"]]
    assert h[77] == 127 and set(np.delete(h, 77).tolist()) == {0, 2} and ref["inv_s"][special["half"]] == 1.0
    assert np.array_equal(ref["a"][special["half_neg"]], -h)
    assert np.array_equal(ref["a"][special["big"]], ref["a"][0]) and np.array_equal(ref["a"][special["small"]], ref["a"][0])
    assert ref["a"][special["spike"]][1023] == -127 and not ref["a"][special["zero"]].any()
    assert ref["delta"][special["zero"]] == 0.0 and ref["delta"][special["spike"]] > 0.0
    nq = qf.shape[0]
    qa = lay.qa(ws).cpu().numpy()
    a_nat = qa[:, _ph2_perm()] if mode == "binary" else qa
    assert np.array_equal(a_nat[:nq], ref["a"]), np.nonzero((a_nat[:nq] != ref["a"]).any(1))[0]
    if mode == "binary":
        assert not np.array_equal(qa[:nq], ref["a"])          # ... and binary really is permuted
    delta, alpha, beta = lay.delta(ws), lay.alpha(ws), lay.beta(ws)
    err = np.abs(delta[:nq] - ref["delta"])
    assert np.all(err <= 1e-12 * ref["delta"]), (np.argmax(err), err.max())
    assert np.array_equal(alpha[:nq], ref["alpha"])
    assert np.all(np.abs(beta[:nq] - ref["beta"]) <= ref["beta_tol"])
    if mode != "binary":
        assert not beta.any()
    # padding queries: zero pieces, zero bound and map, and a threshold nothing passes
    assert not qa[nq:].any() and not delta[nq:].any() and not alpha[nq:].any() and not beta[nq:].any()
    thr = lay.thr(ws)
    assert np.all(np.isposinf(thr[nq:])) and not np.isposinf(thr[:nq]).any()


# ------------------------------------------------------------------------------------------------
# 2. sample pass
def _dv_reference(lay, a, c):
    """max of u over the rows of every (query, sample chunk, lane): f64 [nq, scols], NaN where a lane
    holds no row with a value.  a: the checked pieces (natural order), int8 device tensor."""
    dev = a.device
    nsc, T = lay.scols // 32, lay.scr // 32
    idx = (torch.arange(nsc, device=dev)[:, None, None] * lay.sstride + torch.arange(T, device=dev)[None, :, None] * 32
           + torch.arange(32, device=dev)[None, None, :])
    valid = idx < lay.n
    rows = idx.clamp(max=lay.n - 1).reshape(-1)
    if c.mode == "binary":
        u = a.double() @ _bits(c.codes[rows]).double().T                          # exact integers
    else:
        u = (a.double() @ c.x8[rows].double().T) / c.norms[rows][None, :]
        valid = valid & (c.norms[rows].view(nsc, T, 32) > 0)
    u = torch.where(valid.reshape(-1)[None, :], u, torch.full_like(u, -torch.inf)).view(-1, nsc, T, 32).amax(2)
    u = torch.where(torch.isinf(u), torch.full_like(u, torch.nan), u)
    return u.reshape(-1, lay.scols)


@pytest.mark.parametrize("nq", [40, 300])
@pytest.mark.parametrize("n", [8192, 20_000, 70_001])
@pytest.mark.parametrize("mode", ["binary", "int8_cosine"])
def test_sample_pass_lane_maxima(dev, mode, n, nq):
    SAMPLE, _, _ = _stage()
    g = torch.Generator(device=dev).manual_seed(n + nq)
    k = 10
    if mode == "binary":
        c = Corpus(mode, dev, codes=torch.randint(0, 256, (n, 128), generator=g, device=dev, dtype=torch.uint8))
    else:
        x8 = torch.randint(-127, 128, (n, D), generator=g, device=dev, dtype=torch.int8)
        x8[::61] = 0                                         # zero-norm rows: u is NaN
        x8[32:64] = 0                                        # (lane 0..31 of sample chunk 0: fewer rows, or none)
        c = Corpus(mode, dev, x8=x8)
    qf = torch.randn((nq, D), generator=g, device=dev)
    lay = Layout(mode, n, nq, k)
    T = lay.scr // 32
    nsc = lay.scols // 32
    if n == 8192 and nq <= 256:
        assert T == 1 and nsc * 32 == n and lay.sstride == 32        # every row is its own lane maximum
    if n == 20_000:
        assert T > 1 and (nsc - 1) * lay.sstride + lay.scr >= n      # shared lanes; the sample is every row
    if n == 70_001:
        assert nsc * lay.scr < n and lay.sstride > lay.scr           # a strict subset
    _, ws = _call(c, qf, k, SAMPLE)
    ref = M.prep_reference(mode, qf.cpu().numpy())
    a = _pieces(lay, ws, mode)
    assert np.array_equal(a.cpu().numpy(), ref["a"])
    want = _dv_reference(lay, a, c)
    dv = lay.dv(ws).double()
    assert torch.equal(torch.isnan(dv), torch.isnan(want))
    if mode == "int8_cosine" and T == 1:
        assert bool(torch.isnan(want).any())                         # a lane of zero-norm rows only
    fin = ~torch.isnan(want)
    if mode == "binary":
        assert torch.equal(dv[fin], want[fin])
    else:
        assert bool((torch.abs(dv[fin] - want[fin]) <= 2.0 ** -20 * want[fin].abs() + 1e-30).all())


@pytest.mark.parametrize("mode", ["binary", "int8_cosine"])
def test_sample_pass_ragged_last_chunk(dev, mode):
    """A last sample chunk cut at n to a length that is no multiple of 32: its last tile is shifted back
    to end at n, so a lane holds other rows than lane + 32 t there.  What the select's proof needs still
    holds: the chunk's maxima are values of distinct rows of the chunk, i.e. sorted descending they are
    dominated by the chunk's sorted u, and the largest is the chunk's maximum.  Every other chunk follows
    the lane rule."""
    SAMPLE, _, _ = _stage()
    n, nq, k = 20_010, 40, 10
    g = torch.Generator(device=dev).manual_seed(n)
    if mode == "binary":
        c = Corpus(mode, dev, codes=torch.randint(0, 256, (n, 128), generator=g, device=dev, dtype=torch.uint8))
    else:
        x8 = torch.randint(-127, 128, (n, D), generator=g, device=dev, dtype=torch.int8)
        x8[::61] = 0
        c = Corpus(mode, dev, x8=x8)
    qf = torch.randn((nq, D), generator=g, device=dev)
    lay = Layout(mode, n, nq, k)
    nsc = lay.scols // 32
    r0 = (nsc - 1) * lay.sstride
    nrows = n - r0
    assert 32 < nrows < lay.scr and nrows % 32 != 0
    _, ws = _call(c, qf, k, SAMPLE)
    a = _pieces(lay, ws, mode)
    want = _dv_reference(lay, a, c)
    dv = lay.dv(ws).double()
    head = slice(0, (nsc - 1) * 32)
    assert torch.equal(torch.isnan(dv[:, head]), torch.isnan(want[:, head]))
    band = 0.0 if mode == "binary" else 2.0 ** -20
    fin = ~torch.isnan(want[:, head])
    assert bool((torch.abs(dv[:, head][fin] - want[:, head][fin]) <= band * want[:, head][fin].abs()).all())
    if mode == "binary":
        u = a.double() @ _bits(c.codes[r0:n]).double().T
    else:
        u = (a.double() @ c.x8[r0:n].double().T) / c.norms[r0:n][None, :]
        u = torch.where(c.norms[r0:n][None, :] > 0, u, torch.full_like(u, -torch.inf))
    top = torch.sort(u, dim=1, descending=True).values[:, :32]
    last = dv[:, (nsc - 1) * 32:]
    assert not bool(torch.isnan(last).any())                 # (two rows per lane at most, one of them with a norm)
    got = torch.sort(last, dim=1, descending=True).values
    assert bool((got <= top + band * top.abs()).all())
    assert bool((torch.abs(got[:, 0] - top[:, 0]) <= band * top[:, 0].abs()).all())
    if mode == "binary":                                     # each maximum is the value of a row of the chunk
        assert bool((last[:, :, None] == u[:, None, :]).any(2).all())


# ------------------------------------------------------------------------------------------------
# 3. select kernel
def _expected_thr(dv, delta, k):
    """thr of every query from the kernel's own dv and Delta: U by a sort."""
    U = np.array([M.kth_largest(dv[q], k) for q in range(dv.shape[0])])
    return U, M.round_down_f32(U - 2.0 * delta[:dv.shape[0]])


def _assert_thr(lay, ws, k):
    dv = lay.dv(ws).cpu().numpy()
    U, want = _expected_thr(dv, lay.delta(ws), k)
    thr = lay.thr(ws)
    assert np.array_equal(thr[:lay.nq].view(np.uint32), want.view(np.uint32)), (thr[:lay.nq], want)
    assert np.all(np.isposinf(thr[lay.nq:]))
    return dv, U


@pytest.mark.parametrize("k", [1, 10, 1024])
@pytest.mark.parametrize("case", ["top22", "top11", "equal"])
def test_select_threshold_vs_sort(dev, case, k):
    SAMPLE, _, _ = _stage()
    n = 8192
    v = M.select_values(case, n, seed=k)
    c = Corpus("binary", dev, codes=M.rows_for_values(v))
    w = M.value_query()
    qf = np.stack([w, -w, np.zeros(D, np.float32)])
    lay = Layout("binary", n, 3, k)
    _, ws = _call(c, qf, k, SAMPLE)
    dv, U = _assert_thr(lay, ws, k)
    assert np.array_equal(np.sort(dv[0]), np.sort(v.astype(np.float32)))       # every row is a lane maximum
    assert U[0] > 0 and U[1] < 0 and U[2] == 0 and not np.signbit(U[2])
    assert np.all(dv[2] == 0)                                                 # (all values equal, and U = +0)
    # the radix passes are decided where the case says: more than k values share U's top key bits
    key, ku = M.float_key(dv[0]), M.float_key(np.float32(U[0]))
    share = {"top22": 10, "top11": 21, "equal": 0}[case]
    assert int((key >> share == ku >> share).sum()) >= k + 1
    if case == "top22":
        assert len(np.unique(key[key >> 10 == ku >> 10])) == 8
    if case == "top11":
        assert len(np.unique(key[key >> 21 == ku >> 21] >> 10)) > 500


@pytest.mark.parametrize("k", [1, 10, 1024])
def test_select_threshold_too_few_values(dev, k):
    """Fewer than k finite sample values -> thr = -inf (every row a candidate); as many as k -> finite."""
    SAMPLE, _, _ = _stage()
    rng = np.random.default_rng(31)
    n = 8192
    x8 = np.zeros((n, D), np.int8)
    live = np.sort(rng.permutation(n)[:7])
    x8[live] = rng.integers(-127, 128, (7, D))
    c = Corpus("int8_cosine", dev, x8=x8)
    qf = rng.standard_normal((5, D)).astype(np.float32)
    lay = Layout("int8_cosine", n, 5, k)
    _, ws = _call(c, qf, k, SAMPLE)
    dv, U = _assert_thr(lay, ws, k)
    assert int((~np.isnan(dv[0])).sum()) == 7
    assert np.all(np.isneginf(lay.thr(ws)[:5])) == (k > 7) and np.all(np.isfinite(lay.thr(ws)[:5])) == (k <= 7)
    # Phase II has no NaN: a corpus of fewer than k rows
    cb = Corpus("binary", dev, codes=rng.integers(0, 256, (500, 128), dtype=np.uint8))
    layb = Layout("binary", 500, 5, k)
    _, wsb = _call(cb, qf, k, SAMPLE)
    dvb, Ub = _assert_thr(layb, wsb, k)
    assert int((~np.isnan(dvb[0])).sum()) == 500
    assert np.all(np.isneginf(layb.thr(wsb)[:5])) == (k > 500)


# ------------------------------------------------------------------------------------------------
# 4. soundness on adversarial inputs
RATIO_FLOOR = {"binary_sym": 0.99, "binary_asym": 0.99, "int8_cosine": 0.93}   # (test_gemm_bound_model.py)


def _fixture_corpus(fx, dev):
    if fx["mode"] == "binary":
        return Corpus("binary", dev, codes=fx["codes"])
    if fx["mode"] == "int8_cosine":
        return Corpus("int8_cosine", dev, x8=fx["x8"])
    return Corpus("float_ip", dev, xf=fx["F"])


@pytest.mark.parametrize("name", M.FIXTURES)
def test_adversarial_fixture_served_exactly(dev, name, lib=None):
    """The matrix path alone (no fallback; the lists cannot overflow: 32-row chunks) returns the
    oracle's rows, order and scores although the victim's u is the lowest of the must-rows by
    nearly 2 Delta."""
    _, _, NOFB = _stage()
    fx = M.fixture(name)
    c = _fixture_corpus(fx, dev)
    lay = Layout(fx["mode"], c.n, fx["qf"].shape[0], fx["k"], lib)
    assert lay.chunk_rows == 32 < lay.capc
    res, _ = _call(c, fx["qf"], fx["k"], NOFB, lib=lib)
    _check_oracle(c, fx["qf"], fx["k"], res, codes=fx.get("codes"), x8=fx.get("x8"), F=fx.get("F"))
    assert res[1][0, 0] == fx["victim"] and np.array_equal(res[1][0, 1:], fx["winners"][:fx["k"] - 1])


@pytest.mark.parametrize("name", M.FIXTURES)
def test_adversarial_fixture_bound_holds_and_is_reached(dev, name, lib=None):
    """Delta >= max |u - s'| with the GPU's own u (dv: at this size one row per lane) and Delta, s' in
    float64; and the fixtures reach the bound to the floors their CPU model test confirms."""
    SAMPLE, _, _ = _stage()
    fx = M.fixture(name)
    mode, nq = fx["mode"], fx["qf"].shape[0]
    c = _fixture_corpus(fx, dev)
    lay = Layout(mode, c.n, nq, fx["k"], lib)
    assert lay.scr == 32 and lay.sstride == 32 and lay.scols == c.n
    _, ws = _call(c, fx["qf"], fx["k"], SAMPLE, lib=lib)
    bounds = None
    if mode == "float_ip":
        x8, _, bref = M.flat_prepare_reference(fx["F"])
        bounds = c.bounds.cpu().numpy()
        assert np.array_equal(c.x8.cpu().numpy(), x8)
        assert np.all(bounds >= bref) and np.all(bounds <= bref * (1 + 1e-9) + 1e-290)
    prep = M.prep_reference(mode, fx["qf"], bounds)
    assert np.array_equal(_pieces(lay, ws, mode).cpu().numpy(), prep["a"])
    u = lay.dv(ws).double().cpu().numpy()
    sp = M.scores_u_units(mode, fx["qf"], prep, fx.get("codes"), fx.get("x8"), fx.get("F"))
    delta = lay.delta(ws)[:nq]
    fin = ~np.isnan(u) & np.isfinite(sp)
    assert np.array_equal(~fin, np.isneginf(sp)) and int(fin.sum()) > 0.98 * fin.size
    gap = np.where(fin, np.abs(u - np.where(fin, sp, 0.0)), 0.0).max(axis=1)
    ratio = gap / delta
    print(f"{name}: max|u - s'| / Delta = {ratio}")
    assert np.all(delta >= gap)
    assert np.all(delta >= prep["delta"] * (1 - 1e-12))       # (a smaller Delta is wrong even where unreached)
    if name in RATIO_FLOOR:
        assert np.all(ratio >= RATIO_FLOOR[name])
    # the threshold the select kernel set admits the victim, and by less than the room the proof leaves
    thr = lay.thr(ws)
    uv, uw = u[0, fx["victim"]], u[0, fx["winners"][0]]
    assert uw - 2 * delta[0] - 1e-3 * delta[0] <= thr[0] <= uw - 2 * delta[0] and uv >= thr[0]


# ------------------------------------------------------------------------------------------------
# 5. scale and range
def _clustered(rng, n, nclus=16):
    C = rng.standard_normal((nclus, D)) / 32.0
    F = C[rng.integers(0, nclus, n)] + (0.6 / 32.0) * rng.standard_normal((n, D))
    return (F / np.linalg.norm(F, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def scale_data():
    rng = np.random.default_rng(55)
    n, nq = 6000, 24
    F = _clustered(rng, n)
    codes, x8, _ = O.encode_batch("cohere", F, 0.1)
    qf = F[rng.integers(0, n, nq)] + (0.3 / 32.0) * rng.standard_normal((nq, D))
    qf = (qf / np.linalg.norm(qf, axis=1, keepdims=True)).astype(np.float32)
    S = {m: O.exhaustive_scores(m, qf, codes=codes, x8=x8) for m in ("binary", "int8_cosine")}
    return dict(F=F, codes=codes, x8=x8, qf=qf, S=S)


@pytest.mark.parametrize("mode", ["binary", "int8_cosine"])
def test_query_scale_is_exact(dev, scale_data, mode):
    """Queries scaled by 2^60 and 2^-60: the same pieces bit for bit, the same rows, and the scores
    scaled exactly."""
    _, _, NOFB = _stage()
    d, k = scale_data, 10
    qf, nq = d["qf"], d["qf"].shape[0]
    c = Corpus(mode, dev, codes=d["codes"], x8=d["x8"])
    batch = np.concatenate([qf, qf * np.float32(2.0 ** 60), qf * np.float32(2.0 ** -60)])
    lay = Layout(mode, c.n, 3 * nq, k)
    (cnt, rows, sc), ws = _call(c, batch, k, NOFB)
    ref = O.exhaustive_topk(d["S"][mode], k)
    assert np.all(cnt == k)
    for j, f in enumerate((1.0, 2.0 ** 60, 2.0 ** -60)):
        assert np.array_equal(rows[j * nq:(j + 1) * nq], ref), j
        assert np.array_equal(sc[j * nq:(j + 1) * nq], np.take_along_axis(d["S"][mode], ref, 1) * f), j
    a = lay.qa(ws).cpu().numpy()
    assert np.array_equal(a[:nq], a[nq:2 * nq]) and np.array_equal(a[:nq], a[2 * nq:3 * nq]) and a[:nq].any()
    delta = lay.delta(ws)
    assert np.allclose(delta[:nq], delta[nq:2 * nq], rtol=1e-12) and np.allclose(delta[:nq], delta[2 * nq:3 * nq],
                                                                                  rtol=1e-12)


@pytest.mark.parametrize("mode", ["binary", "int8_cosine"])
def test_subnormal_queries_vs_oracle(dev, scale_data, mode):
    """Every query component a float32 subnormal (or zero): the oracle on those float32 values is the
    definition."""
    d, k = scale_data, 10
    qf = (d["qf"].astype(np.float64) * 2.0 ** -124).astype(np.float32)
    tiny = np.finfo(np.float32).tiny
    assert np.all(np.abs(qf) < tiny) and np.all(np.abs(qf).max(axis=1) > 0)
    c = Corpus(mode, dev, codes=d["codes"], x8=d["x8"])
    res, _ = _call(c, qf, k, 0)
    _check_oracle(c, qf, k, res, codes=d["codes"], x8=d["x8"])


# ------------------------------------------------------------------------------------------------
# 6. retry pass at the smallest n whose chunks can overflow
def _smallest_overflowable_n(mode, nq, k):
    """The smallest n the plan gives chunks of at least twice the list capacity (a 700-row cluster then
    fits one chunk and overflows its list)."""
    def ok(n):
        lay = Layout(mode, n, nq, k)
        return lay.chunk_rows >= 2 * lay.capc
    lo, hi = 1, 1 << 24
    assert ok(hi) and not any(ok(1 << e) for e in range(5, 19))
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid) else (mid + 1, hi)
    assert ok(lo) and not ok(lo - 1)
    return lo


CLUSTER = 720


def _retry_corpus(mode, n, qf, lo, dev, g):
    """Random background rows and, in rows [lo, lo + CLUSTER), a cluster graded from background level
    (first) to near-identical to query 0 (last)."""
    q0 = qf[0]
    if mode == "binary":
        codes = torch.randint(0, 256, (n, 128), generator=g, device=dev, dtype=torch.uint8)
        p = torch.linspace(0.5, 0.0, CLUSTER, device=dev)
        flip = torch.rand((CLUSTER, D), generator=g, device=dev) < p[:, None]
        bits = ((q0 > 0)[None, :] ^ flip).view(CLUSTER, 128, 8).to(torch.uint8)
        sh = torch.arange(7, -1, -1, device=dev, dtype=torch.uint8)
        codes[lo:lo + CLUSTER] = (bits << sh).sum(2).to(torch.uint8)
        return Corpus(mode, dev, codes=codes)
    x8 = torch.empty((n, D), dtype=torch.int8, device=dev)
    for r0 in range(0, n, 1 << 16):
        r1 = min(n, r0 + (1 << 16))
        x8[r0:r1] = torch.round(38.0 * torch.randn((r1 - r0, D), generator=g, device=dev)).clamp(-127, 127).to(torch.int8)
    a = torch.round(q0 * (127.0 / q0.abs().max()))
    w = torch.linspace(0.0, 1.0, CLUSTER, device=dev)[:, None]
    noise = 38.0 * torch.randn((CLUSTER, D), generator=g, device=dev)
    x8[lo:lo + CLUSTER] = torch.round(w * a[None, :] + torch.sqrt(1 - w * w) * noise).clamp(-127, 127).to(torch.int8)
    return Corpus(mode, dev, x8=x8)


def _device_scores(c, qf):
    """The oracle's score of every row (oracle.exhaustive_scores restated in float64 torch; the queries
    sit on a 2^-12 grid, so every float64 dot is exact in any summation order)."""
    q64 = qf.double()
    out = torch.empty((qf.shape[0], c.n), dtype=torch.float64, device=c.dev)
    for r0 in range(0, c.n, 1 << 16):
        r1 = min(c.n, r0 + (1 << 16))
        if c.mode == "binary":
            out[:, r0:r1] = q64 @ (2.0 * _bits(c.codes[r0:r1]).double() - 1.0).T
        else:
            x = c.x8[r0:r1].double()
            out[:, r0:r1] = (q64 @ x.T).float().double() / x.pow(2).sum(1).sqrt()[None, :]
    return out


@pytest.mark.parametrize("mode", ["binary", "int8_cosine"])
def test_retry_pass_serves_an_overflowed_chunk(dev, mode, lib=None):
    SAMPLE, MAIN, NOFB = _stage()
    nq, k = 8, 10
    n = _smallest_overflowable_n(mode, nq, k)
    lay = Layout(mode, n, nq, k, lib)
    cr, capc = lay.chunk_rows, lay.capc
    assert cr >= 2 * capc and CLUSTER > capc and CLUSTER <= cr and n <= 1 << 21
    # a main-pass chunk that no sample chunk touches (sample chunk c: rows [c * sstride, + scr))
    s0 = np.arange(lay.scols // 32) * lay.sstride
    free = [m for m in range(1, lay.nchunks - 1) if not np.any((s0 < (m + 1) * cr) & (s0 + lay.scr > m * cr))]
    m = free[len(free) // 2]
    lo = (m + 1) * cr - CLUSTER                     # the best cluster rows are the chunk's last
    g = torch.Generator(device=dev).manual_seed(606)
    qf = (torch.round(1024.0 * torch.randn((nq, D), generator=g, device=dev)) / 4096.0).contiguous()
    c = _retry_corpus(mode, n, qf, lo, dev, g)
    # precondition: the cluster overflows the (query 0, chunk m) list of the main pass
    ws = torch.zeros((lay.bytes,), dtype=torch.uint8, device=dev)
    for st in (SAMPLE, MAIN):
        _call(c, qf, k, st, ws, lib)
    cnt = lay.cnt(ws).cpu().numpy()
    assert cnt[0, m] > capc, (cnt[0, m], capc)
    assert np.all(np.delete(cnt[0], m) <= capc) and np.all(cnt[1:] <= capc)
    # the full call without the fallback: reachable only through the retry pass
    (count, rows, sc), _ = _call(c, qf, k, NOFB, ws, lib)
    S = _device_scores(c, qf)
    sub = [torch.arange(lo, lo + CLUSTER, device=dev)]
    for q in range(nq):
        kth = torch.topk(S[q], k).values[-1]
        cand = torch.nonzero(S[q] >= kth).flatten()
        sub.append(cand)
        cs, cn = S[q][cand].cpu().numpy(), cand.cpu().numpy()
        o = np.lexsort((cn, -cs))[:k]
        assert count[q] == k
        assert np.array_equal(rows[q], cn[o]), (mode, q)
        assert np.array_equal(sc[q], cs[o]), (mode, q)
    assert np.all(rows[0] >= lo + CLUSTER - 128) and np.all(rows[0] < lo + CLUSTER)
    # ... and the restated scores are the oracle's, on the rows that decide the result
    sub = torch.unique(torch.cat(sub))
    if mode == "binary":
        So = O.exhaustive_scores(mode, qf.cpu().numpy(), codes=c.codes[sub].cpu().numpy())
    else:
        So = O.exhaustive_scores(mode, qf.cpu().numpy(), x8=c.x8[sub].cpu().numpy())
    assert np.array_equal(So, S[:, sub].cpu().numpy())
