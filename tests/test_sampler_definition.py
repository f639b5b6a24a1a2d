"""The sampler's definition (tests/sampler_cases.py) held to the oracle's LVC_Process on the synthetic caches, and the Python
restatement of the guided draw held to the literal bisection.  No GPU: this keeps the REFERENCE of
tests/test_gpu_sampler_synthetic.py honest and says nothing about the device.

Both sides of the first comparison sum a subspace's weights one after the other in double precision (the oracle with
set_cmf_double(True), the product's accumulation precision), so there is no tolerance: integers, CMFs and sum_pmf bit for bit."""
import numpy as np
import pytest

from tests import sampler_cases as sc

SEED = 20240607


@pytest.fixture(scope="module")
def caches(pkg):
    return sc.cases(np.random.default_rng(SEED))


@pytest.fixture(scope="module")
def oracle(pkg, ob):
    o = ob.Oracle(pkg.scenes.cornell_box())
    o.set_cmf_double(True)
    return o


def test_the_case_list_is_what_it_says(caches):
    assert [len(caches[f"random_{n}"]) for n in sc.RANDOM_N] == list(sc.RANDOM_N)
    for name, c in caches.items():
        n = len(c)
        assert c.dtype == sc.light_vertex_dtype() and (c["path_id"] == np.arange(n)).all(), name
        if n:
            assert c["subspace_id"].min() >= 0 and c["subspace_id"].max() < sc.NUM_SUBSPACE, name
        pdf = c["pdf"][c["pdf"] != 0]
        assert (np.frexp(pdf)[0] == 0.5).all(), name              # powers of two
    size = lambda name: np.bincount(caches[name]["subspace_id"], minlength=sc.NUM_SUBSPACE)
    assert size("one_subspace_5000")[999] == 5000
    assert (size("every_id_once") == 1).all()
    for name in ("run_lengths", "zero_run_lengths"):
        assert tuple(size(name)[np.arange(len(sc.RUN_LENGTHS)) * 90]) == sc.RUN_LENGTHS and size(name).sum() == sum(sc.RUN_LENGTHS)
    ids = caches["lanes_mod_64"]["subspace_id"].reshape(-1, 64)
    assert (np.sort(ids, axis=1) == np.arange(64)).all()           # 64 different ids in every wave
    assert (np.diff(caches["lanes_ascending"]["subspace_id"].astype(int)) >= 0).all() and caches["lanes_ascending"]["subspace_id"][-1] == 999
    assert (np.diff(caches["lanes_descending"]["subspace_id"].astype(int)) <= 0).all()
    for name in ("zero_subspace", "zero_second_half", "zero_first_half"):
        c = caches[name]
        assert len(c) == 3000 and len(np.unique(c["subspace_id"])) == 6
        w, mine = sc.weights(c), c["subspace_id"] == 334
        half = np.arange(3000) >= 1500
        zero = {"zero_subspace": mine, "zero_second_half": mine & half, "zero_first_half": mine & ~half}[name]
        assert zero.sum() > 100 and (w[zero] == 0).all() and (w[~zero] > 0).mean() > 0.999
    w = sc.weights(caches["dynamic_range"]).astype(np.float64)
    assert w[w > 0].max() / w[w > 0].min() > 1e50 and len(np.unique(caches["dynamic_range"]["subspace_id"])) == 40
    c = caches["nan_inf"]
    assert (c["pdf"][::5] == 0).all() and np.isinf(c["flux"][::7]).any(axis=1).all() and np.isnan(c["flux"][::11]).any(axis=1).all()
    assert len(caches["empty"]) == 0


def test_definition_equals_the_oracle_bit_for_bit(caches, oracle):
    for name, cache in caches.items():
        jump, size, bias, cmf, sum_pmf, vc, pc = sc.definition(cache)
        oracle.lvc_import(cache)
        oracle.build_sampler()
        sub, ocmf, ojump, ovc, opc = oracle.sampler_read(capacity=max(len(cache), 1))
        assert (ovc, opc) == (vc, pc), name
        np.testing.assert_array_equal(sub["size"], size, err_msg=name)
        np.testing.assert_array_equal(sub["jump_bias"], bias, err_msg=name)
        np.testing.assert_array_equal(ojump, jump, err_msg=name)
        assert np.isfinite(cmf).all(), name
        np.testing.assert_array_equal(ocmf.view(np.uint32), cmf.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(sub["sum_pmf"].view(np.uint32), sum_pmf.view(np.uint32), err_msg=name)
        for s in np.flatnonzero(size):
            c = cmf[bias[s]:bias[s] + size[s]]
            assert c[-1] == 1.0 and (np.diff(c) >= 0).all(), (name, s)


def test_vectorised_bisection_is_the_literal_one(caches):
    rng = np.random.default_rng(SEED + 1)
    for name in ("run_lengths", "zero_run_lengths", "random_65"):
        jump, size, bias, cmf, *_ = sc.definition(caches[name])
        for s in np.flatnonzero(size):
            c = cmf[bias[s]:bias[s] + size[s]]
            u = sc.draw_values(c, rng, cap=40, randoms=10)[::7]
            k, pmf = sc.bisection(c, u)
            for x, kk, pp in zip(u, k, pmf):
                want = sc.reference_bisection(c, x)
                assert kk == want and pp.view(np.uint32) == (c[want] if want == 0 else c[want] - c[want - 1]).view(np.uint32), (name, s, x)


def test_window_walk_restated_equals_the_bisection(caches):
    """guide entry, c0 = max(g - 1, 0), pos = (bias + c0) & ~3, the masks of guide_window, stop at an entry above u -- against
    binary_sample, bin and pmf bits, for every non-empty subspace of the run-length and zero-weight caches (7 000+ draws)."""
    rng = np.random.default_rng(SEED + 2)
    draws = multi = 0
    for name in sc.WALK_CASES:
        jump, size, bias, cmf, *_ = sc.definition(caches[name])
        guide_all = np.zeros(len(cmf), np.int64)
        for s in np.flatnonzero(size):
            guide_all[bias[s]:bias[s] + size[s]] = sc.guide(cmf[bias[s]:bias[s] + size[s]])
        for s in np.flatnonzero(size):
            b, m = int(bias[s]), int(size[s])
            u = sc.draw_values(cmf[b:b + m], rng)
            k, pmf = sc.bisection(cmf[b:b + m], u)
            wk, wpmf, windows = sc.window_walk(cmf, guide_all, b, m, u)
            np.testing.assert_array_equal(wk, k, err_msg=f"{name} {s}")
            np.testing.assert_array_equal(wpmf.view(np.uint32), pmf.view(np.uint32), err_msg=f"{name} {s}")
            draws += len(u)
            multi += int((windows > 1).sum())
    assert draws > 7000 and multi > 0, (draws, multi)
