"""The light-vertex sampler by its definition, and the synthetic caches it is held to: shared by tests/test_sampler_definition.py
(the definition against the oracle's LVC_Process, no GPU) and tests/test_gpu_sampler_synthetic.py (the device build and the guided
second-stage draw against the definition).  Not a conftest: plain functions, imported where they are used.

The definition (csrc/kernels_sampler.hip builds the same tables with a counting sort, a tiled double-precision scan and a copy):
  weight     w = ((flux0 + flux1) + flux2) / pdf in FP32, NaN / +-inf -> 0             (LVCSubspaceInfoCopy, device_thrust.cu:191-212)
  jump       stable argsort of the subspace ids: inside a subspace the cache's own order
  size       vertices per id; jump_bias = exclusive running sum (an empty subspace carries the running offset)
  cmf        per subspace a sequential FP64 running sum of its weights in cache order, divided by the total and rounded to FP32;
             a subspace whose total is not > 0 samples uniformly, cmf[j] = float32(j + 1) / float32(size); the last entry is 1
  sum_pmf    float32(total)
  path_count vertices of depth 0
"""
import numpy as np

from tests.test_gpu_sampling_tables import reference_bisection, reference_guide

NUM_SUBSPACE = 1000
CONNECTION_N = 3
U_STEP = 2.0 ** -24          # rnd() returns the multiples of 2^-24 in [0, 1)


def light_vertex_dtype():
    import __graft_entry__ as g
    return g.load_package().LIGHT_VERTEX_DTYPE


def weights(cache):
    f = np.asarray(cache["flux"], np.float32)
    with np.errstate(all="ignore"):
        w = ((f[:, 0] + f[:, 1]) + f[:, 2]) / np.asarray(cache["pdf"], np.float32)
    assert w.dtype == np.float32
    w[~np.isfinite(w)] = 0.0
    return w


def definition(cache):
    """(jump, size, jump_bias, cmf, sum_pmf, vertex_count, path_count) of a cache of LIGHT_VERTEX_DTYPE."""
    n = len(cache)
    ids = np.asarray(cache["subspace_id"], np.int64)
    assert n == 0 or (ids.min() >= 0 and ids.max() < NUM_SUBSPACE)
    w = weights(cache).astype(np.float64)
    jump = np.argsort(ids, kind="stable").astype(np.int32)
    size = np.bincount(ids, minlength=NUM_SUBSPACE).astype(np.int32)
    jump_bias = (np.cumsum(size) - size).astype(np.int32)
    cmf = np.zeros(n, np.float32)
    sum_pmf = np.zeros(NUM_SUBSPACE, np.float32)
    for s in np.flatnonzero(size):
        b, m = int(jump_bias[s]), int(size[s])
        run = np.cumsum(w[jump[b:b + m]])          # (add.accumulate: one addition after the other, in cache order)
        total = run[-1]
        if total > 0.0:
            c = (run / total).astype(np.float32)
        else:
            c = np.arange(1, m + 1).astype(np.float32) / np.float32(m)
        c[-1] = 1.0
        cmf[b:b + m] = c
        sum_pmf[s] = np.float32(total)
    return jump, size, jump_bias, cmf, sum_pmf, n, int((np.asarray(cache["depth"]) == 0).sum())


def guide(cmf):
    """The second-stage guide table of one subspace (tests/test_gpu_sampling_tables.py: reference_guide)."""
    return reference_guide(cmf)


def bisection(cmf, u):
    """binary_sample (cuProg.h:245-264) as written, for an array of random numbers at once: (bin, pmf).  The loop is the bisection
    of reference_bisection, every draw taking its own branch (tests/test_sampler_definition.py holds the two to each other)."""
    cmf = np.asarray(cmf, np.float32)
    u = np.atleast_1d(np.asarray(u, np.float32))
    size = len(cmf)
    lo = np.zeros(len(u), np.int64)
    hi = np.full(len(u), size, np.int64)
    mid = np.full(len(u), size // 2 - 1, np.int64)
    while True:
        live = hi - lo > 1
        if not live.any():
            break
        less = u < cmf[np.clip(mid, 0, size - 1)]
        hi = np.where(live & less, mid + 1, hi)
        lo = np.where(live & ~less, mid + 1, lo)
        mid = (lo + hi) // 2 - 1
    pmf = np.where(lo == 0, cmf[lo], cmf[lo] - cmf[np.maximum(lo - 1, 0)]).astype(np.float32)
    return lo, pmf


def window_walk(cmfs, guide_all, bias, size, u, window=8):
    """The guided draw (csrc/second_stage_guided.inc.h, dev_sampling.h: guide_window) restated: the guide entry of the random
    number's bucket, c0 = max(g - 1, 0), aligned windows of eight entries from (bias + c0) & ~3 on, of which the places
    [bias + c0, bias + size) take part, until an entry is above u.  `cmfs` / `guide_all` are the WHOLE tables (a window reads the
    neighbouring subspaces' entries and masks them).  (bin, pmf, windows read)."""
    u = np.atleast_1d(np.asarray(u, np.float32))
    pad = np.concatenate([np.asarray(cmfs, np.float32), np.full(window, 0.5, np.float32)])   # (the device allocates n + 8)
    end = bias + size
    bucket = np.minimum((u * np.float32(size)).astype(np.int32), size - 1)
    g = np.asarray(guide_all)[bias + bucket].astype(np.int64)
    c0 = np.maximum(g - 1, 0)
    first = bias + c0
    pos = first & ~3
    cnt = c0.copy()
    lo = np.full(len(u), -np.inf, np.float32)
    hi = np.full(len(u), np.inf, np.float32)
    live = np.ones(len(u), bool)
    windows = np.zeros(len(u), np.int64)
    while live.any():
        for i in range(window):
            at = pos + i
            v = pad[np.minimum(at, len(pad) - 1)]
            take = live & ((i >= 3) | (at >= first)) & (at < end)
            le = take & (v <= u)
            gt = take & ~(v <= u)
            cnt = cnt + le
            lo = np.where(le, np.maximum(lo, v), lo)
            hi = np.where(gt, np.minimum(hi, v), hi)
        windows += live
        pos = np.where(live, pos + window, pos)
        live = live & ~(hi < np.inf) & (pos < end)
    cmf = pad[bias:end]
    over = cnt >= size                      # no entry above u: the bisection's last bin
    k = np.where(over, size - 1, cnt)
    with np.errstate(invalid="ignore"):
        inside = np.where(k == 0, hi, hi - lo)
    last = np.where(k == 0, cmf[k], cmf[k] - cmf[np.maximum(k - 1, 0)])
    return k, np.where(over, last, inside).astype(np.float32), windows


def snap(u):
    """into the value set of rnd(): clipped to [0, 1 - 2^-24], rounded DOWN to a multiple of 2^-24"""
    u = np.clip(np.asarray(u, np.float64), 0.0, 1.0 - U_STEP)
    return (np.floor(u / U_STEP) * U_STEP).astype(np.float32)


def draw_values(cmf, rng, cap=2000, randoms=50):
    """The random numbers a subspace is drawn with: every CMF entry and the number below it, every bucket boundary j / size and the
    number below it (at most `cap` evenly spaced j), 0, 1 - 2^-24 and `randoms` uniform ones."""
    size = len(cmf)
    c = np.asarray(cmf, np.float64)
    j = np.arange(size) if size <= cap else np.unique(np.linspace(0, size - 1, cap).astype(np.int64))
    b = j / size
    return snap(np.concatenate([c, c - U_STEP, b, b - U_STEP, [0.0, 1.0 - U_STEP], rng.random(randoms)]))


# ---- the caches ---------------------------------------------------------------------------------------------------------------
RANDOM_N = (1, 63, 64, 65, 511, 512, 513, 32767, 32768, 32769, 40000)     # a wave, the 512 chunks of the build, 512 x 64
RUN_LENGTHS = (255, 256, 257, 511, 512, 513, 1, 2, 7, 8, 9)              # the 256-wide tiles of the CMF scan; ids 0, 90, 180, ...
LANE_N = 4096


def make_cache(ids, w, rng, pdf=None):
    """A cache with the given subspace ids and weights: path_id = index, pdf a power of two (1 unless given), the flux split
    0.5 / 0.25 / 0.25 of w * pdf, depth random in {0, 1, 2}; every other field random, so that each record's 96 bytes are its own."""
    n = len(ids)
    c = np.zeros(n, light_vertex_dtype())
    pdf = np.ones(n, np.float32) if pdf is None else np.asarray(pdf, np.float32)
    t = np.asarray(w, np.float32) * pdf
    c["flux"] = t[:, None] * np.array([0.5, 0.25, 0.25], np.float32)[None, :]
    c["pdf"] = pdf
    c["subspace_id"] = ids
    c["depth"] = rng.integers(0, 3, n)
    c["path_id"] = np.arange(n, dtype=np.uint32)
    c["pad"] = (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    for name in ("position", "normal", "color", "last_position"):
        c[name] = rng.random((n, 3), np.float32)
    for name in ("single_pdf", "rmis_pointer", "last_lum", "last_normal_projection"):
        c[name] = rng.random(n, np.float32)
    c["material_id"] = rng.integers(0, 8, n)
    c["last_zone_id"] = rng.integers(0, NUM_SUBSPACE, n)
    return c


def _runs(rng):
    ids = np.concatenate([np.full(m, 90 * k) for k, m in enumerate(RUN_LENGTHS)])
    return rng.permutation(ids)


def _over(ids_of, n, rng):
    return np.asarray(ids_of)[rng.integers(0, len(ids_of), n)]


def cases(rng):
    """name -> cache, in a fixed order (a dict).  Ids within 0 .. 999 only."""
    out = {}
    for n in RANDOM_N:
        out[f"random_{n}"] = make_cache(rng.integers(0, NUM_SUBSPACE, n), rng.random(n) * 4.0, rng)
    out["one_subspace_5000"] = make_cache(np.full(5000, 999), rng.random(5000) * 4.0, rng)
    out["every_id_once"] = make_cache(rng.permutation(NUM_SUBSPACE), rng.random(NUM_SUBSPACE) * 4.0, rng)
    ids = _runs(rng)
    out["run_lengths"] = make_cache(ids, rng.random(len(ids)) * 4.0, rng)
    i = np.arange(LANE_N)
    up = i * NUM_SUBSPACE // LANE_N
    for name, ids in (("lanes_mod_64", i % 64), ("lanes_mod_2", i % 2), ("lanes_ascending", up), ("lanes_descending", up[::-1].copy())):
        out[name] = make_cache(ids, rng.random(LANE_N) * 4.0, rng)
    six = (0, 5, 333, 334, 700, 999)
    for name in ("zero_subspace", "zero_second_half", "zero_first_half"):
        n = 3000
        ids = _over(six, n, rng)
        w = rng.random(n) * 4.0
        hit = ids == 334
        if name == "zero_second_half":
            hit &= np.arange(n) >= n // 2
        if name == "zero_first_half":
            hit &= np.arange(n) < n // 2
        w[hit] = 0.0
        out[name] = make_cache(ids, w, rng)
    ids = _runs(rng)
    w = rng.random(len(ids)) * 4.0
    w[rng.random(len(ids)) < 0.5] = 0.0
    for k in range(len(RUN_LENGTHS)):            # ... and each run ends in a tail of 1e-12 (the last fifth of it, at least one vertex)
        at = np.flatnonzero(ids == 90 * k)
        w[at[-max(1, len(at) // 5):]] = 1e-12
    out["zero_run_lengths"] = make_cache(ids, w, rng)
    n = 4000
    out["dynamic_range"] = make_cache(_over(np.arange(40) * 25 + 7, n, rng), 10.0 ** rng.uniform(-30, 30, n), rng,
                                      pdf=2.0 ** rng.integers(-20, 20, n))
    n = 2000
    c = make_cache(_over(np.arange(10) * 111, n, rng), rng.random(n) * 4.0, rng)
    c["pdf"][::5] = 0.0
    c["flux"][::7, 0] = np.inf
    c["flux"][::11, 1] = np.nan
    out["nan_inf"] = c
    out["empty"] = make_cache(np.zeros(0, np.int64), np.zeros(0), rng)
    return out


DRAW_CASES = ("run_lengths", "zero_subspace", "zero_second_half", "zero_first_half", "zero_run_lengths", "every_id_once",
              "one_subspace_5000", "lanes_mod_64", "random_40000", "random_1")
WALK_CASES = ("run_lengths", "zero_subspace", "zero_second_half", "zero_first_half", "zero_run_lengths")


def build_order(names):
    """The order the device builds them in on ONE context: the largest first, then one vertex, then 513 -- stale tables of a larger
    build under a smaller one -- the rest, and the largest again."""
    head = ["random_40000", "random_1", "random_513"]
    return head + [n for n in names if n not in head] + ["random_40000"]


__all__ = ["definition", "guide", "bisection", "window_walk", "draw_values", "cases", "snap", "reference_bisection"]
