"""The device sampler build and the guided second-stage draw on synthetic caches (tests/sampler_cases.py), against the sampler's
definition -- which tests/test_sampler_definition.py holds to the oracle bit for bit.  The caches are imported with lvc_import, so
every size and every id pattern is chosen: around a wave (63 / 64 / 65), around the 512 chunks of the counting sort (511 / 512 /
513, 512 x 64 +- 1), subspaces of 255 .. 513 vertices (the 256-wide tiles of k_sb_cmf and their carry), 64 different ids in a wave
and one id in all of them, id 999, zero-weight heads and tails, NaN / inf weights, 60 decades of weights, an empty cache, and a
small build after a large one on the same context.

  (a) counting-sort build (k_sb_hist / k_sb_scan / k_sb_scatter / k_sb_cmf / k_sb_copy): vertex and path count, size, jump_bias of
      all 1000 subspaces and the jump buffer EXACT; every CMF entry finite, non-decreasing, ending in 1.0, within one FP32 ulp of
      the definition and >= 99.9 % of them bit-identical; sum_pmf within one ulp; the guide table equal to its definition on the
      device's own CMF; the sorted cache (SPCBPT_UNIT_SORTED) byte for byte cache[jump[i]].
      The CMF bound: both sides add non-negative weights in double; the device's 256-wide tile scan and the sequential sum differ
      by at most ~n 2^-53 = 4e-12 relative, so the FP32 roundings differ only where the quotient lies that close to a rounding
      boundary (an expected share of 1e-4), and then by one ulp.
      Measured (MI355X, 25 builds, 221 563 CMF entries of subspaces with a positive total): 0 not bit-identical (share 0), max 0 ulp;
      sum_pmf bit-identical.
  (b) radix-sort build (SPCBPT_SAMPLER_BUILD=hipcub, the cross-check form): the same integer tables and sorted cache, the CMFs
      within the 1.5e-7 absolute that test_counting_sampler_build_gives_the_tables_of_the_radix_sort grants between the two forms.
      Without the 60-decade cache: this form takes differences of ONE double prefix over the whole cache, so a subspace 1e8 times
      lighter than the cache loses digits (kernels_sampler.hip: k_cmf).  Measured: max |difference| 1.7e-15 (the cache with
      tails of 1e-12), 0 on the 23 other builds.
  (c) the draw the eye megakernel runs (SPCBPT_UNIT_STAGE2_GUIDED: csrc/second_stage_guided.inc.h, the text k_spcbpt compiles):
      for every non-empty subspace of ten caches and random numbers ON every CMF entry, just below it, on and below every bucket
      boundary, 0, 1 - 2^-24 and 50 random ones, three draws a record (same subspace / mixed / one slot empty): size, bin, place in
      the sorted cache and pmf bits equal to the literal bisection on the device's own CMF.  No allowance.  Measured: 479 022 draws,
      0 mismatches; 64 188 in the first bin, 63 213 in the last, 87 through more than one window (bin - guide entry >= 8), 1 527
      subspaces that start off a quad boundary, 480 empty slots.
"""
import numpy as np
import pytest

from tests import sampler_cases as sc
from tests.test_gpu_units import OP     # include/spcbpt.h: spcbpt_unit_op

pytestmark = pytest.mark.gpu

SEED = 20240607
STAGE2_GUIDED, SORTED = OP["STAGE2_GUIDED"], OP["SORTED"]


@pytest.fixture(scope="module")
def caches(pkg):
    return sc.cases(np.random.default_rng(SEED))


@pytest.fixture(scope="module")
def definitions(caches):
    return {name: sc.definition(c) for name, c in caches.items()}


def _renderer(pkg):
    r = pkg.Renderer(pkg.scenes.cornell_box(), 0)
    r.set_subspace()
    return r


@pytest.fixture(scope="module")
def counting(gpu, pkg):
    return _renderer(pkg)


def _build(r, cache):
    r.lvc_import(cache)
    r.build_sampler()
    n = max(len(cache), 1)
    sub, cmfs, jump, vc, pc = r.sampler_read(capacity=n)
    guide2, _, _ = r.sampling_tables(vc)
    return sub, cmfs, jump, vc, pc, guide2


def _check_integers_and_structure(name, r, cache, want, got):
    """What both build forms owe: the integer tables exact, the CMFs' structure, the guide table by its definition on the device's
    own CMF, the sorted cache byte for byte.  Returns the mask of the CMF entries whose subspace has a positive total."""
    jump, size, bias, cmf, sum_pmf, vc, pc = want
    sub, dcmf, djump, dvc, dpc, dguide = got
    assert (dvc, dpc) == (vc, pc), name
    np.testing.assert_array_equal(sub["size"], size, err_msg=name)
    np.testing.assert_array_equal(sub["jump_bias"], bias, err_msg=name)
    np.testing.assert_array_equal(djump, jump, err_msg=name)
    assert np.isfinite(dcmf).all(), name
    positive = np.zeros(vc, bool)
    for s in np.flatnonzero(size):
        b, m = int(bias[s]), int(size[s])
        c = dcmf[b:b + m]
        assert c[-1] == 1.0 and (np.diff(c) >= 0).all(), (name, s)
        if sum_pmf[s] > 0:
            positive[b:b + m] = True
        else:   # float32(j + 1) / float32(size), which is what the definition holds there
            np.testing.assert_array_equal(c.view(np.uint32), cmf[b:b + m].view(np.uint32), err_msg=f"{name} {s}")
        np.testing.assert_array_equal(dguide[b:b + m], sc.guide(c), err_msg=f"{name} {s}")
    if vc:
        rec = r.unit(SORTED, np.arange(vc, dtype=np.uint32).reshape(-1, 1), 24)
        np.testing.assert_array_equal(rec, np.ascontiguousarray(cache[jump]).view(np.uint32).reshape(vc, 24), err_msg=name)
    return positive


def test_counting_build_is_the_definition(counting, caches, definitions):
    r = counting
    entries = differing = 0
    worst = 0.0
    for name in sc.build_order(list(caches)):
        want, got = definitions[name], _build(r, caches[name])
        positive = _check_integers_and_structure(name, r, caches[name], want, got)
        cmf, dcmf = want[3][positive], got[1][positive]
        err = np.abs(dcmf.astype(np.float64) - cmf.astype(np.float64))
        ulp = np.spacing(cmf).astype(np.float64)
        same = int((dcmf.view(np.uint32) == cmf.view(np.uint32)).sum())
        entries += len(cmf); differing += len(cmf) - same
        if len(cmf):
            worst = max(worst, float((err / ulp).max()))
            print(f"{name}: {len(cmf)} CMF entries, {len(cmf) - same} not bit-identical, max {float((err / ulp).max()):.2f} ulp")
        assert (err <= ulp).all(), (name, float((err / ulp).max()))
        assert same >= 0.999 * len(cmf), (name, same, len(cmf))
        sp, dsp = want[4], got[0]["sum_pmf"]
        assert (np.abs(dsp.astype(np.float64) - sp.astype(np.float64)) <= np.spacing(sp).astype(np.float64)).all(), name
    print(f"counting build: {entries} CMF entries, {differing} not bit-identical ({differing / max(entries, 1):.2e}), max {worst:.2f} ulp")
    assert entries > 200000


def test_radix_sort_build_gives_the_same_tables(counting, caches, definitions, pkg, monkeypatch):
    monkeypatch.setenv("SPCBPT_SAMPLER_BUILD", "hipcub")
    r2 = _renderer(pkg)
    monkeypatch.delenv("SPCBPT_SAMPLER_BUILD")
    worst = 0.0
    for name in sc.build_order([n for n in caches if n != "dynamic_range"]):
        got2 = _build(r2, caches[name])
        _check_integers_and_structure(name, r2, caches[name], definitions[name], got2)
        got = _build(counting, caches[name])
        if len(got[1]):
            d = float(np.abs(got2[1].astype(np.float64) - got[1].astype(np.float64)).max())
            worst = max(worst, d)
            print(f"{name}: radix-sort CMF - counting CMF, max {d:.3g}")
        np.testing.assert_allclose(got2[1], got[1], rtol=0, atol=1.5e-7, err_msg=name)
    print(f"radix-sort build: max CMF difference to the counting build {worst:.3g}")


def test_guided_draw_is_the_bisection(counting, caches):
    r = counting
    rng = np.random.default_rng(SEED + 3)
    seen = dict(draws=0, first_bin=0, last_bin=0, multi_window=0, unaligned=0, empty_slots=0)
    for name in sc.DRAW_CASES:
        sub, cmfs, jump, vc, pc, guide2 = _build(r, caches[name])
        size, bias = sub["size"].astype(np.int64), sub["jump_bias"].astype(np.int64)
        sid, u, ek, epmf, eg = [], [], [], [], []
        for s in np.flatnonzero(size):
            b, m = int(bias[s]), int(size[s])
            c = cmfs[b:b + m]
            x = sc.draw_values(c, rng)
            k, pmf = sc.bisection(c, x)
            sid.append(np.full(len(x), s)); u.append(x); ek.append(k); epmf.append(pmf)
            eg.append(guide2[b + np.minimum((x * np.float32(m)).astype(np.int32), m - 1)].astype(np.int64))
            seen["unaligned"] += int(b % 4 != 0)
        sid, u, ek, epmf, eg = (np.concatenate(a) for a in (sid, u, ek, epmf, eg))
        n = len(u)
        # three draws a record: in order (mostly one subspace, of one size), mixed (a third of them again, shuffled: three subspaces,
        # three sizes, three window counts), and records that name an empty subspace in slot 0, 1 or 2
        in_order = np.resize(np.arange(n), (n + 2) // 3 * 3).reshape(-1, 3)
        mixed = rng.permutation(n)[:max(n // 9, 1) * 3] if n >= 3 else np.zeros(0, np.int64)
        at = np.concatenate([in_order, mixed.reshape(-1, 3)])
        ids, ubits = sid[at].astype(np.uint32), u[at].view(np.uint32)
        empty = np.flatnonzero(size == 0)
        if len(empty):
            extra = rng.integers(0, n, (60, 3))
            slot = np.arange(60) % 3
            e_ids, e_u = sid[extra].astype(np.uint32), u[extra].view(np.uint32)
            e_ids[np.arange(60), slot] = empty[rng.integers(0, len(empty), 60)]
            extra[np.arange(60), slot] = -1
            at, ids, ubits = np.concatenate([at, extra]), np.concatenate([ids, e_ids]), np.concatenate([ubits, e_u])
        out = r.unit(STAGE2_GUIDED, np.concatenate([ids, ubits], axis=1), 4 * sc.CONNECTION_N).reshape(-1, sc.CONNECTION_N, 4)
        got_size, got_k, got_slot, got_pmf = (out[..., i].astype(np.int32 if i < 3 else np.uint32) for i in range(4))
        live = at >= 0
        a = at[live]
        np.testing.assert_array_equal(got_size[live], size[sid[a]], err_msg=name)
        np.testing.assert_array_equal(got_k[live], ek[a], err_msg=name)
        np.testing.assert_array_equal(got_pmf[live], epmf[a].view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(got_slot[live], bias[sid[a]] + ek[a], err_msg=name)
        # an empty subspace is skipped: size 0, no bin, no place, pmf 0 -- and its neighbours in the record were checked above
        assert (got_size[~live] == 0).all() and (got_k[~live] == -1).all() and (got_slot[~live] == -1).all() and (got_pmf[~live] == 0).all(), name
        seen["draws"] += int(live.sum()); seen["empty_slots"] += int((~live).sum())
        seen["first_bin"] += int((ek == 0).sum()); seen["last_bin"] += int((ek == size[sid] - 1).sum())
        seen["multi_window"] += int((ek - eg >= 8).sum())
    print("guided draw:", seen)
    assert seen["draws"] > 10 ** 4 and all(v > 0 for v in seen.values()), seen
