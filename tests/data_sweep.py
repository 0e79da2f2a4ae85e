"""The case matrix of tests/test_gpu_data_sweep.py: shapes (proposals, observations, forced mapping) that put the data-density kernels
(kmc_data.hpp) and their planner (kmc_data.hip: data_plan) on every edge of their tree -- both mappings, chosen and forced
(KMC_DEBUG=data-map); observation counts either side of a chunk, a wave and a workgroup block; 1, 2, 4, 8 and 16 or more rounds per
wave, up to the stack's full depth (4096); 1 to 4 populated waves in the last block; a padded chunk of 1, some and 15 real rows; block
counts that are no power of two, and 2048; proposal counts that leave the last wave of lanes nearly empty.  `plan` restates the
planner, `last_block` what the end of the data then looks like, `CELLS` names every cell the matrix must reach, and `reference` is the
value contract in numpy (the body's operation order, then the pairwise tree).  No GPU is needed here:

    python tests/data_sweep.py

prints the plan of every case and which cases reach each cell, runs the reference of every case and checks that it could tell a
differently ordered sum apart, and exits non-zero if a cell is missed, a case is vacuous or a reference is too large.  The GPU module
asserts `plan` against Sampler.describe(), so the restatement cannot drift from the library.

Rounds 4096 in the proposal-per-lane mapping needs 65 537 proposals over 131 073 observations, 8.6e9 terms; LANE_DEEP is that case,
(65 600, 131 073).  One evaluation of it measured 6 ms on an MI355X, copies included (its test 0.03 s with the numpy reference of 16
rows), so it stays; rounds 4096 in the other mapping, (1025, 524 289), measured 3 ms."""
import functools
import os
import sys
from collections import OrderedDict, namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_data_density_cpu import REG_TERM, pairwise  # noqa: E402  (REG_TERM: re-exported for the GPU module)

# kmc_data.hpp / kmc_data.hip
WAVES, CHUNK, LEVELS, TARGET_GROUPS, LANE_FROM = 4, 16, 13, 2048, 512
RMAX = 1 << (LEVELS - 1)

ND, P0 = 2, 4.0                     # the sweep's one kernel: REG_TERM at ndim = ncols = 2, precision p[0]
FULL_ROWS = 2_000_000               # the reference covers every row up to this many terms, else SUBSET_ROWS rows
SUBSET_ROWS = 16
MAX_TERMS = 20_000_000              # ... and never more than this many terms at once (160 MB of doubles)

Plan = namedtuple("Plan", "mapping rounds nblocks groups")
Last = namedtuple("Last", "waves wave_obs chunks fill mod64")
Case = namedtuple("Case", "nprop ndata force")


def plan(nprop, ndata, force=None):
    """data_plan: the mapping ("obs": one observation per lane, one proposal per workgroup; "lane": one proposal per lane), the rounds
    per wave, the blocks of observations, and the workgroups along x."""
    assert force in (None, "lane", "obs")
    obs = (nprop < LANE_FROM) if force is None else force == "obs"
    chunk = 64 if obs else CHUNK
    groups = nprop if obs else (nprop + 63) // 64

    def blocks(r):
        b = WAVES * chunk * r
        return (ndata + b - 1) // b

    r = 1
    while r < RMAX and (blocks(r) > 4096 or (groups * blocks(r) > TARGET_GROUPS and blocks(r) > 1)):
        r *= 2
    return Plan("obs" if obs else "lane", r, blocks(r), groups)


def last_block(nprop, ndata, force=None):
    """The last block of observations under plan(): its populated waves (1 .. 4), the observations and chunks (rounds run) of the last
    populated wave, the real rows of that wave's last chunk (`fill`: 64 or 16 when whole), and nprop mod 64."""
    p = plan(nprop, ndata, force)
    chunk = 64 if p.mapping == "obs" else CHUNK
    per_wave = chunk * p.rounds
    left = ndata - (p.nblocks - 1) * WAVES * per_wave
    assert 1 <= left <= WAVES * per_wave
    waves = -(-left // per_wave)
    wave_obs = left - (waves - 1) * per_wave
    chunks = -(-wave_obs // chunk)
    return Last(waves, wave_obs, chunks, wave_obs - (chunks - 1) * chunk, nprop % 64)


def describe_words(nprop, ndata, force=None, tempered=False):
    """What Sampler.describe() says of a half-step of `nprop` proposals under this plan."""
    p = plan(nprop, ndata, force)
    head = "data_partial_obs (one observation per lane, grid " if p.mapping == "obs" else "data_partial_lane (one proposal per lane, grid "
    return [head + "%d x %d workgroups of 256, %d rounds per wave)" % (p.groups, p.nblocks, p.rounds), "data_fold_split" if tempered else "data_fold ->"]


LANE_DEEP = Case(65600, 131073, "lane")
CASES = [Case(*c) for c in [
    # the smallest trees, and the ends of a chunk (16), a wave (64) and a block (64 lane, 256 obs)
    (1, 1, None), (2, 2, None), (3, 3, None), (511, 63, None), (20, 64, None), (20, 65, None), (7, 255, None), (512, 256, "obs"), (600, 257, "obs"),
    (1, 1, "lane"), (63, 2, "lane"), (65, 3, "lane"), (1, 15, "lane"), (63, 16, "lane"), (575, 17, None), (512, 63, None), (576, 64, None),
    (65, 65, "lane"), (64, 47, "lane"), (64, 130, "lane"), (128, 400, "lane"),
    # populated waves and block counts in the observation-per-lane mapping
    (5, 129, None), (5, 193, None), (9, 520, None), (2, 1300, None), (40, 7000, None),
    # rounds per wave
    (511, 5000, None), (300, 3000, None), (400, 10000, None), (20, 30000, None), (1000, 2900, "obs"), (700, 3457, "obs"), (1, 524288, None), (1, 1048577, None),
    (2000, 20001, "obs"), (1025, 524289, "obs"),
    (3000, 3001, None), (4096, 5000, None), (4096, 4977, None), (16384, 2065, None), (16384, 1921, None), (16384, 2287, None), (8192, 12289, None), (8192, 11953, None),
    (2048, 2049, None), (64, 131072, "lane"), (63, 4097, "lane"), (5000, 1409, None), LANE_DEEP,
]]


def case_id(c):
    return "%dx%d%s" % (c.nprop, c.ndata, "-" + c.force if c.force else "")


def other_mapping(c):
    return "lane" if plan(*c).mapping == "obs" else "obs"


# ---- coverage -----------------------------------------------------------------------------------------------------------
def _popcount(n):
    return bin(n).count("1")


def _rounds_class(r):
    return "16+" if r >= 16 else str(r)


def _cells():
    """name -> predicate(case, plan, last).  Both mappings wherever a cell is one of the kernels'."""
    cells = OrderedDict()
    cells["mapping: obs chosen at nprop 511"] = lambda c, p, l: c.force is None and c.nprop == 511 and p.mapping == "obs"
    cells["mapping: lane chosen at nprop 512"] = lambda c, p, l: c.force is None and c.nprop == 512 and p.mapping == "lane"
    for n in (1, 63, 65):
        cells["mapping: lane forced at nprop %d" % n] = lambda c, p, l, n=n: c.force == "lane" and c.nprop == n
    cells["mapping: obs forced at nprop >= 512"] = lambda c, p, l: c.force == "obs" and c.nprop >= 512
    for m, sizes in (("lane", (1, 2, 3, 15, 16, 17, 63, 64, 65)), ("obs", (1, 2, 3, 63, 64, 65, 255, 256, 257))):
        for n in sizes:
            cells["%s: ndata %d" % (m, n)] = lambda c, p, l, m=m, n=n: p.mapping == m and c.ndata == n
        cells["%s: one observation past a whole block, rounds > 1" % m] = \
            lambda c, p, l, m=m: p.mapping == m and p.rounds > 1 and p.nblocks > 1 and l.waves == 1 and l.wave_obs == 1
        for r in ("1", "2", "4", "8", "16+"):
            cells["%s: rounds %s" % (m, r)] = lambda c, p, l, m=m, r=r: p.mapping == m and _rounds_class(p.rounds) == r
            if r != "1":
                cells["%s: rounds %s, last wave ragged" % (m, r)] = \
                    lambda c, p, l, m=m, r=r: p.mapping == m and _rounds_class(p.rounds) == r and l.wave_obs < (64 if m == "obs" else CHUNK) * p.rounds
        cells["%s: last wave's chunk count has two bits set" % m] = lambda c, p, l, m=m: p.mapping == m and _popcount(l.chunks) == 2
        cells["%s: last wave's chunk count has three or more bits set" % m] = lambda c, p, l, m=m: p.mapping == m and _popcount(l.chunks) >= 3
        for w in (1, 2, 3, 4):
            cells["%s: %d populated waves in the last block" % (m, w)] = lambda c, p, l, m=m, w=w: p.mapping == m and l.waves == w
        for name, ok in (("1", lambda b: b == 1), ("2", lambda b: b == 2), ("3", lambda b: b == 3), ("5", lambda b: b == 5), ("6 or 7", lambda b: b in (6, 7)),
                         ("two-digit odd", lambda b: 10 <= b <= 99 and b % 2 == 1), ("2048", lambda b: b == 2048)):
            cells["%s: nblocks %s" % (m, name)] = lambda c, p, l, m=m, ok=ok: p.mapping == m and ok(p.nblocks)
    cells["obs: rounds 4096"] = lambda c, p, l: p.mapping == "obs" and p.rounds == RMAX
    cells["lane: rounds 4096"] = lambda c, p, l: p.mapping == "lane" and p.rounds == RMAX
    for name, ok in (("1 real row", lambda f: f == 1), ("2 .. 14 real rows", lambda f: 2 <= f <= 14), ("15 real rows", lambda f: f == 15)):
        cells["lane: padded chunk of %s" % name] = lambda c, p, l, ok=ok: p.mapping == "lane" and ok(l.fill)
        cells["lane: padded chunk of %s after whole chunks" % name] = lambda c, p, l, ok=ok: p.mapping == "lane" and ok(l.fill) and l.chunks > 1
    cells["obs: last round of 1 real row"] = lambda c, p, l: p.mapping == "obs" and l.fill == 1
    cells["obs: last round of 63 real rows"] = lambda c, p, l: p.mapping == "obs" and l.fill == 63
    for r in (0, 1, 63):
        cells["lane: nprop mod 64 = %d" % r] = lambda c, p, l, r=r: p.mapping == "lane" and l.mod64 == r
    cells["obs: nprop 1"] = lambda c, p, l: p.mapping == "obs" and c.nprop == 1
    return cells


CELLS = _cells()


def coverage(cases=None):
    """cell name -> the ids of the cases that reach it."""
    cases = CASES if cases is None else cases
    return OrderedDict((name, [case_id(c) for c in cases if hit(c, plan(*c), last_block(*c))]) for name, hit in CELLS.items())


# ---- inputs and the reference -------------------------------------------------------------------------------------------
def reg_data(ndata, nd, seed):
    """Observations of a linear model and its coefficients (as tests/test_gpu_data_density.py: reg_data)."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((ndata, nd - 1))
    beta = np.linspace(0.5, -0.5, nd)
    y = beta[0] + Z @ beta[1:] + 0.5 * rng.standard_normal(ndata)
    return np.column_stack([Z, y]), beta


def reg_terms(X, D, p0):
    """REG_TERM for every (row, observation), in the body's operation order."""
    n = X.shape[1]
    mu = np.repeat(X[:, 0:1], D.shape[0], axis=1)
    for k in range(1, n):
        mu = mu + X[:, k:k + 1] * D[None, :, k - 1]
    r = D[None, :, n - 1] - mu
    return -0.5 * p0 * r * r


@functools.lru_cache(maxsize=2)
def _data(ndata, seed):
    return reg_data(ndata, ND, seed)


def inputs(c, extra=0):
    """The case's observations and rows (near the regression solution); `extra` > 0: another, independent set of rows."""
    D, beta = _data(c.ndata, 7 * c.ndata + c.nprop)
    X = beta + 0.05 * np.random.default_rng(1000003 * extra + c.nprop).standard_normal((c.nprop, ND))
    return D, X


def check_rows(nprop, ndata):
    """The rows the reference is computed for: all of them while that is at most FULL_ROWS terms, else at most SUBSET_ROWS: the first,
    the last, and the rows either side of multiples of 64 (the last ones first: where a wave of lanes ends)."""
    if nprop * ndata <= FULL_ROWS:
        return np.arange(nprop)
    rows = [0, nprop - 1]
    k = (nprop - 1) // 64 * 64
    edges = []
    while k > 0:
        edges += [k, k - 1]
        k -= 64
    pick = edges[:6] + edges[-6:] + edges[len(edges) // 2 - 1:len(edges) // 2 + 1]
    for r in pick:
        if r not in rows and len(rows) < SUBSET_ROWS:
            rows.append(r)
    return np.array(sorted(rows))


def reference(term_fn, prior_fn, X, D):
    """The value contract: prior(x) + the pairwise tree over term(x, d_j) in index order, -inf where the prior is -inf.
    `term_fn(X, D) -> [rows, ndata]` in the body's operation order; `prior_fn(X) -> [rows]` or None."""
    with np.errstate(all="ignore"):
        S = pairwise(np.asarray(term_fn(X, D), dtype=np.float64))
        if prior_fn is None:
            return 0.0 + S
        pri = np.asarray(prior_fn(X), dtype=np.float64)
        return np.where(pri == -np.inf, -np.inf, pri + S)


def reg_reference(X, D):
    return reference(lambda X_, D_: reg_terms(X_, D_, P0), None, X, D)


# ---- vacuity: sums in another order -------------------------------------------------------------------------------------
def sequential(T):
    """The plain left-to-right sum of each row."""
    return np.cumsum(T, axis=1)[:, -1]


def blocked(T, size=48):
    """The tree cut into blocks of `size` terms that are not aligned powers of two: pairwise inside each, then over the blocks."""
    return pairwise(np.column_stack([pairwise(T[:, j:j + size]) for j in range(0, T.shape[1], size)]))


def vacuity(c, other=sequential, min_rows=64):
    """(rows where `other` gives different bits from the pairwise tree, rows checked) over the case's own data: its reference rows,
    and for a case that has fewer than `min_rows` proposals, independent sets of rows until that many were checked."""
    D, X = inputs(c)
    X = X[check_rows(c.nprop, c.ndata)]
    extra = 0
    while c.nprop < min_rows and X.shape[0] < min_rows:
        extra += 1
        X = np.concatenate([X, inputs(c, extra)[1]])
    step = max(1, MAX_TERMS // c.ndata)
    differ = 0
    for i in range(0, X.shape[0], step):
        T = reg_terms(X[i:i + step], D, P0)
        differ += int(np.sum(pairwise(T) != other(T)))
    return differ, X.shape[0]


def main():
    import time
    bad = 0
    print("%-22s %-5s %6s %7s %7s  %5s %9s %6s %4s  %5s  %s" % ("case", "map", "rounds", "nblocks", "groups", "waves", "wave obs", "chunks", "fill", "mod64", "pairwise != sequential"))
    t_all = time.time()
    for c in CASES:
        p, l = plan(*c), last_block(*c)
        t0 = time.time()
        D, X = inputs(c)
        rows = check_rows(c.nprop, c.ndata)
        want = reg_reference(X[rows], D)
        note = ""
        if rows.size * c.ndata > MAX_TERMS or not np.all(np.isfinite(want)):
            bad += 1
            note = "REFERENCE TOO LARGE OR NOT FINITE"
        if c.ndata >= 17:
            d, n = vacuity(c)
            note += "%d of %d rows" % (d, n)
            if 10 * d < n:
                bad += 1
                note += " VACUOUS"
        print("%-22s %-5s %6d %7d %7d  %5d %9d %6d %4d  %5d  %s  (%.2f s)" % (case_id(c), p.mapping, p.rounds, p.nblocks, p.groups, l.waves, l.wave_obs, l.chunks, l.fill,
                                                                              l.mod64, note, time.time() - t0))
    print()
    for name, ids in coverage().items():
        print("%-62s %s" % (name, ", ".join(ids) if ids else "MISSING"))
        bad += not ids
    print("%d cases, %d cells, %d problems, %.0f s" % (len(CASES), len(CELLS), bad, time.time() - t_all))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
