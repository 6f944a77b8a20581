"""CPU test of tests/gemm_bound_model.py: the adversarial fixtures of tests/test_gpu_gemm_bound.py keep
their teeth.  This is a condition on the fixtures, not a measurement of the kernel: the float64 model of
K5's rule (pieces, Delta, U over all rows, thr = U - 2 Delta) keeps every row of the exact top-k, and
each weakening that the GPU tests are there to catch makes the model lose one.

Which weakening a fixture can show follows from its construction (S = 1; rp / rn = the one-sided
residual sums): the winners overstate their score by rn, the victim understates its by rp, and the
victim is lost once 2 Delta' < rp + rn.
  binary_sym   rp = rn = 225: Delta' = 0.9 Delta loses it (405 < 450), and so does thr = U - Delta
  binary_asym  rp = 270, rn = 180: min(rp, rn) loses it (360 < 450); 0.9 Delta cannot (486 > 450: no
               input with these two sums can), which is why the symmetric fixture exists
  int8_cosine  ||rho|| = 14.23, winners + 13.3, victim - 14.2: 0.9 Delta loses it (25.6 < 27.5)
  float_ip     both terms of the bound are Cauchy-Schwarz products and one row has 8 times the norm of
               the others, so the bound is far from attained: kept, and the ratio is only reported
"""
import numpy as np
import pytest

import gemm_bound_model as M


@pytest.mark.parametrize("name", M.FIXTURES)
def test_fixture_is_what_it_claims(name):
    fx = M.fixture(name)
    kept, must, ratio = M.model_keeps(fx)
    # query 0: the victim is the single best row, the other k - 1 places go to the first winners, and
    # the k-th score is tied among the k winners: k + 1 must-rows
    want = np.zeros(kept.shape[1], bool)
    want[fx["victim"]] = True
    want[fx["winners"]] = True
    assert np.array_equal(must[0], want)
    prep = M.prep_reference(fx["mode"], fx["qf"], fx.get("bounds"))
    u = M.matrix_values(fx["mode"], prep["a"], fx.get("codes"), fx.get("x8"), fx.get("scales"))
    sp = M.scores_u_units(fx["mode"], fx["qf"], prep, fx.get("codes"), fx.get("x8"), fx.get("F"))
    assert np.nanargmax(sp[0]) == fx["victim"]
    assert M.kth_largest(u[0], fx["k"]) == u[0, fx["winners"][0]] > u[0, fx["victim"]]
    assert np.all(np.abs(prep["inv_s"] - 1.0) == 0)           # max|q| = 127: q/S = q exactly


@pytest.mark.parametrize("name", M.FIXTURES)
def test_model_keeps_every_must_row(name):
    kept, must, ratio = M.model_keeps(M.fixture(name))
    assert not (must & ~kept).any()
    assert np.all(ratio <= 1.0)


# floors of max|u - s'| / Delta that tests/test_gpu_gemm_bound.py asserts on the GPU's own u and Delta
RATIO_FLOOR = {"binary_sym": 0.99, "binary_asym": 0.99, "int8_cosine": 0.93}


@pytest.mark.parametrize("name", sorted(RATIO_FLOOR))
def test_model_reaches_the_bound(name):
    kept, must, ratio = M.model_keeps(M.fixture(name))
    print(name, "max|u - s'| / Delta =", ratio)
    assert ratio[0] >= RATIO_FLOOR[name]
    assert ratio[0] <= 1.0


@pytest.mark.parametrize("name", ["binary_sym", "int8_cosine"])
def test_smaller_delta_loses_the_victim(name):
    fx = M.fixture(name)
    kept, must, _ = M.model_keeps(fx, scale=0.9)
    assert must[0, fx["victim"]] and not kept[0, fx["victim"]]
    kept, must, _ = M.model_keeps(fx, thr_mult=1.0)           # thr = U - Delta
    assert must[0, fx["victim"]] and not kept[0, fx["victim"]]


def test_binary_sym_loses_the_victim_at_095():
    fx = M.fixture("binary_sym")
    kept, must, _ = M.model_keeps(fx, scale=0.95)
    assert must[0, fx["victim"]] and not kept[0, fx["victim"]]


def test_min_of_the_one_sided_sums_loses_the_victim():
    fx = M.fixture("binary_asym")
    kept, must, _ = M.model_keeps(fx, one_sided=min)
    assert must[0, fx["victim"]] and not kept[0, fx["victim"]]
    kept, must, _ = M.model_keeps(fx, thr_mult=1.0)
    assert must[0, fx["victim"]] and not kept[0, fx["victim"]]
    # the symmetric fixture cannot tell min from max
    kept, must, _ = M.model_keeps(M.fixture("binary_sym"), one_sided=min)
    assert not (must & ~kept).any()


def test_float_fixture_bounds_are_not_attained_by_every_row():
    fx = M.fixture("float_ip")
    x8, s, bounds = M.flat_prepare_reference(fx["F"])
    norms = s * np.sqrt((x8.astype(np.float64) ** 2).sum(1))
    assert np.argmax(norms) == 7 and norms[7] > 4 * np.sort(norms)[-2]
    assert s[fx["victim"]] == 1.0 and np.all(s[fx["winners"]] == 1.0)
    # both terms of the bound carry weight for the victim: the query residual against the row's int8
    # image, and the query against the row's own quantisation residual
    q = fx["qf"][0].astype(np.float64)
    prep = M.prep_reference("float_ip", fx["qf"], bounds)
    t1 = prep["rho"][0] @ (s[fx["victim"]] * x8[fx["victim"]].astype(np.float64))
    t2 = q @ (fx["F"][fx["victim"]].astype(np.float64) - s[fx["victim"]] * x8[fx["victim"]])
    assert t1 > 1000 and t2 > 400


def test_select_value_rows():
    q = M.value_query()
    prep = M.prep_reference("binary", q[None])
    assert np.array_equal(prep["a"][0], q.astype(np.int8)) and not prep["rho"].any()
    for case in ("top22", "top11", "equal"):
        v = M.select_values(case, 8192, seed=3)
        u = M.matrix_values("binary", prep["a"], codes=M.rows_for_values(v))[0]
        assert np.array_equal(u, v)
    key = M.float_key(M.select_values("top22", 8192).astype(np.float32))
    top = np.sort(key)[::-1]
    assert np.all(top[:1100] >> 10 == top[0] >> 10) and len(np.unique(top[:1100])) == 8
    key = M.float_key(M.select_values("top11", 8192).astype(np.float32))
    top = np.sort(key)[::-1]
    assert np.all(top[:2000] >> 21 == top[0] >> 21) and len(np.unique(top[:2000] >> 10)) > 500


def test_float_key_and_round_down():
    v = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    key = M.float_key(v).astype(np.int64)
    assert np.all(np.diff(key) > 0) and M.float_key(np.float32(np.nan)) == 0 and key[0] > 0
    x = np.array([1.0 + 2.0 ** -30, 1.0, -1.0 - 2.0 ** -30, 439.99999999, -np.inf])
    r = M.round_down_f32(x)
    assert np.array_equal(r, np.array([1.0, 1.0, np.nextafter(np.float32(-1), np.float32(-2)),
                                       np.nextafter(np.float32(440), np.float32(0)), -np.inf], np.float32))
