"""GPU: score_kernel (csrc/score.hip) against the high-precision references of oracle/score_hp.py.

* KS numerator h: EXACT against py_oracle.ks_h on the lists py_oracle.score_edges forms (the reference compares Python
  floats), at every storage class of the kernel (LDS 2 x 1024, LDS 2 x 8192, global scratch with the big_off layout of
  either entry point), swap 0 / 1, tie-heavy lists, observations near the 30-bit ceiling, both builds of the kernel.
* Normal branch: the gap lies in the admissible set of the replayed bisection (mpmath conditions, both branches followed
  at a near tie); sd0 no worse than the host's: |dev - hp| <= max(4 |host - hp|, 1e-12 hp), or within the fp64 error
  bound of the closed form where that is larger (the tail of the bracket, where the variance is a small difference).
* Log-normal branch: the gap lies in the admissible set of the replayed two-stage scan (long-double likelihood, direct g),
  for true gaps up to the end of the support, every storage class of the observations and every lanes-per-gap width.
* gap_table_kernel: an entry rounds differently from the mpmath condition only where that lies within its fp64 error
  bound of a rounding boundary.
Near ties met are counted and bounded; the counts are printed (pytest -s)."""
import ctypes as C
import math

import numpy as np
import pytest

from besst_amd import mathstats_compat as MC
from oracle import score_hp as H

pytestmark = pytest.mark.gpu

MU, SIGMA, R = math.log(3000.0), 0.35, 100
CEIL = (1 << 30) - 1                                         # observations are 30-bit in the payload


def builder(edges, node_bits=20):
    """edges: [(obs_lo, obs_hi)] -> DeviceGraphBuilder holding row e = edge e (reduce() of one tuple per link)."""
    import torch
    from besst_amd import pipeline
    keys = np.concatenate([np.full(len(lo), ((((2 * e + 2) << node_bits) | (2 * e + 3)) << 1), np.uint64)
                           for e, (lo, _) in enumerate(edges)])
    lo = np.concatenate([np.asarray(a, np.uint64) for a, _ in edges])
    hi = np.concatenate([np.asarray(b, np.uint64) for _, b in edges])
    assert lo.max() <= CEIL and hi.max() <= CEIL
    payload = lo | ((hi | (np.uint64(3) << np.uint64(30))) << np.uint64(32))
    n = len(keys)
    dev = torch.device('cuda', 0)
    lib = dict(read_len=float(R), ins_size_threshold=1.0e9, min_mapq=11, orientation='fr', detect_duplicate=True,
               extend_paths=True, no_score=False)
    gb = pipeline.DeviceGraphBuilder(dev, 4, node_bits, lib, n, n)
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    gb.reduce(keys=torch.from_numpy(keys.view(np.int64)).to(dev), payload=torch.from_numpy(payload.view(np.int64)).to(dev),
              n_tuples_ptr=C.c_void_p(cnt.data_ptr()), capacity=n)
    torch.cuda.synchronize()
    assert gb.read_sizes()[1] == len(edges)
    assert gb.row_n[:len(edges)].cpu().numpy().view(np.uint32).tolist() == [len(a) for a, _ in edges]
    return gb


# ---- KS numerator -------------------------------------------------------------------------------------------------
KS_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2048, 8191, 8192, 8193, 16384, 16385, 65536 + 3)


def ks_edges(seed):
    rng = np.random.default_rng(seed)
    edges = []
    for n in KS_COUNTS:
        edges.append((rng.integers(100, 3000, n), rng.integers(100, 3000, n)))
    n = 9000
    edges += [
        (np.full(n, 700), np.full(n, 700)),                                   # all equal
        (rng.choice([400, 900], 16400), rng.choice([400, 900], 16400)),        # two values
        (np.arange(20000) % 97 + 200, np.arange(20000) % 97 + 500),            # (x - m1) == (y - m2) for many pairs
        (np.arange(4100) + 100, 4300 - np.arange(4100)),                      # equal means, mirrored
        (rng.integers(CEIL - 5000, CEIL + 1, 9000), rng.integers(CEIL - 3, CEIL + 1, 9000)),   # at the ceiling
        (rng.integers(0, CEIL + 1, 70), rng.integers(0, CEIL + 1, 70)),
        (rng.integers(0, 4, 1500), rng.integers(0, 3, 1500)),
    ]
    return edges


@pytest.fixture(scope='module')
def ks_rows():
    edges = ks_edges(31)
    return edges, builder(edges)


@pytest.mark.parametrize('lognormal', [False, True])
def test_ks_numerator_exact_through_the_builder(ks_rows, lognormal):
    """Every edge in one call, rows out of table order (so the scratch offsets of the big edges are not the trivial ones),
    each row twice with swap 0 and 1."""
    edges, gb = ks_rows
    m = len(edges)
    rng = np.random.default_rng(5)
    big = np.array([e for e in range(m) if len(edges[e][0]) > 8192])
    # every row with swap 0 and 1, then the big rows three times more: adjacent scratch regions of edges that run at once
    rows = np.concatenate([rng.permutation(m), rng.permutation(m), np.tile(rng.permutation(big), 3)]).astype(np.uint32)
    swap = np.concatenate([np.zeros(m), np.ones(m), np.arange(3 * len(big)) % 2]).astype(np.uint8)
    ln = (MU, SIGMA, MC.lognormal_support(MU, SIGMA), 10 ** 6) if lognormal else None
    assert len(big) >= 8 and np.any(np.diff(rows[:m].astype(np.int64)) < 0)
    k = len(rows)
    _, _, ks, _ = gb.score_edges(rows, swap, np.full(k, 40000, np.int32), np.full(k, 40000, np.int32), 3000.0, 300.0, R,
                                 lognormal=ln)
    want = {}
    for i, (r, s) in enumerate(zip(rows, swap)):
        key = (int(r), int(s))
        if key not in want:
            want[key] = H.ks_h(edges[r][0], edges[r][1], int(s))
        assert int(ks[i]) == want[key], (int(r), len(edges[r][0]), int(s), int(ks[i]))


def test_ks_numerator_exact_through_the_context():
    """besst_ctx_score_edges (the C++ big_off layout) on rows of a real graph build: 40 contigs, 1.2 M pairs (edges of
    thousands to tens of thousands of links), both builds."""
    from besst_amd import device, synth
    from oracle import py_oracle as O
    from tests import gpu_util as GU
    asm = synth.make_assembly(40, 6000, 17, sigma_log=0.3, min_len=4000, max_len=12000)
    batch = synth.simulate_library(asm, synth.LibrarySpec('fr', 3000.0, 300.0), 1200000, 18)
    lens = asm.lengths.tolist()
    tab = dict(cls=[1] * asm.nc, scaf=list(range(1, asm.nc + 1)), slen=lens, cpos=[0] * asm.nc, clen=lens,
               cdir=[True] * asm.nc)
    p = O.LibParams(read_len=100, ins_size_threshold=6000.0)
    with device.GraphContext(0) as ctx:
        table, _, _ = GU.device_build(batch, tab, p, ctx=ctx)
        n = table.n.astype(np.int64)
        rows = np.flatnonzero(n >= 1)[::-1]                              # out of table order
        big = rows[n[rows] > 8192]
        assert len(big) >= 2 and (n[rows] <= 8192).sum() >= 2
        # the big rows again, several times over: adjacent scratch regions of edges that run at the same time
        rows = np.concatenate([rows, np.tile(big, 4)]).astype(np.uint32)
        off = table.offset.astype(np.int64)
        lo, hi = table.obs_lo, table.obs_hi
        m = len(rows)
        swap = (np.arange(m) % 2).astype(np.uint8)
        len1 = np.full(m, 40000, np.int32)
        for ln in (None, (MU, SIGMA, MC.lognormal_support(MU, SIGMA), 10 ** 6)):
            gap, _, ks, _ = ctx.score_edges(rows, swap, len1, len1, 3000.0, 300.0, 100.0, lognormal=ln)
            for i, r in enumerate(rows):
                a, b = lo[off[r]:off[r] + n[r]], hi[off[r]:off[r] + n[r]]
                assert int(ks[i]) == H.ks_h(a, b, int(swap[i])), (int(r), int(n[r]))
        # the context's own prefix and tail tables: its log-normal gaps in the admissible set too (a few rows)
        for i in np.argsort(n[rows])[:6]:
            r = rows[i]
            obs = lo[off[r]:off[r] + n[r]].astype(np.int64) + hi[off[r]:off[r] + n[r]]
            assert int(gap[i]) in H.lognormal_gap(MU, SIGMA, 100, obs, 40000, 40000)[0], (int(r), int(n[r]), gap[i])


# ---- normal branch ------------------------------------------------------------------------------------------------
def normal_groups(seed, n_params, per):
    """[((mu, sigma, r), [(c1, c2, n_links, mean_obs)])]: random libraries (fractional r among them), per library edges
    with c1 == c2, c_min < 2r, contigs of 100 kb, the mean observation across the bracket and outside it at both ends."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_params):
        mu = float(rng.uniform(300.0, 6000.0))
        sigma = float(mu * rng.uniform(0.04, 0.25))
        r = float(rng.choice([75.0, 100.0, 100.38, 150.0]))
        lo, hi = int(-4 * sigma), int(mu + 4 * sigma - 2 * r)
        cs = []
        for k in range(per):
            kind = k % 8
            c1, c2 = (int(v) for v in rng.integers(int(2 * sigma) + 1, 40000, 2))
            if kind == 1:
                c2 = c1
            elif kind == 2:
                c1 = int(rng.integers(int(2 * sigma) + 1, int(2 * sigma) + 2 * r + 2))    # c_min < 2r where 2 sigma allows
            elif kind == 3:
                c1 = c2 = 100000
            if kind == 4:
                mean_obs = mu - lo + float(rng.uniform(1, 3 * sigma))                     # gap pinned at the lower end
            elif kind == 5:
                mean_obs = max(1.0, mu - hi - float(rng.uniform(1, 2 * sigma)))           # ... at the upper end
            else:
                mean_obs = max(1.0, float(rng.uniform(mu - hi, mu - lo)))
            cs.append((c1, c2, int(rng.choice([1, 2, 6, 40, 700])), mean_obs))
        out.append(((mu, sigma, r), cs))
    out.append(((500.0, 10.0, 100.0), [(60, 60, 6, 480.0), (60, 60, 3, 700.0)]))        # no placement: g = 0, sd0 = 2^32
    return out


def links_with_total(n, tot):
    a = [tot // n] * n
    for k in range(tot - sum(a)):
        a[k] += 1
    lo = [max(0, o // 3) for o in a]
    return lo, [o - l for o, l in zip(a, lo)]


def test_normal_branch_gap_admissible_and_sigma_no_worse_than_the_host():
    ties = tie_edges = edges_seen = beyond_host = 0
    worst_ratio = 0.0
    for (mu, sigma, r), cs in normal_groups(41, 40, 12):
        links = [links_with_total(n, int(round(mo * n))) for _, _, n, mo in cs]
        gb = builder(links, node_bits=12)
        m = len(cs)
        len1 = np.array([c[0] for c in cs], np.int32)
        len2 = np.array([c[1] for c in cs], np.int32)
        gap, sd0, _, _ = gb.score_edges(np.arange(m, dtype=np.uint32), np.zeros(m, np.uint8), len1, len2, mu, sigma, r)
        for i, (c1, c2, n, _) in enumerate(cs):
            mean_obs = float(sum(links[i][0]) + sum(links[i][1])) / n
            if not (2 * sigma < c1 and 2 * sigma < c2):
                continue
            edges_seen += 1
            adm, t = H.normal_gap(mu, sigma, r, mean_obs, c1, c2)
            ties += t
            tie_edges += t > 0
            assert int(gap[i]) in adm, (mu, sigma, r, c1, c2, n, mean_obs, gap[i], adm)
            hp, err = H.sk_std_dev(mu, sigma, r, c1, c2, int(gap[i]))
            host = MC.tr_sk_std_dev(mu, sigma, r, c1, c2, int(gap[i]))
            if hp >= 2 ** 31 and err == 0.0:
                assert sd0[i] == 2.0 ** 32 == host
                continue
            e_dev, e_host = abs(sd0[i] - hp), abs(host - hp)
            if e_host > 0:
                worst_ratio = max(worst_ratio, e_dev / e_host)
            if e_dev > max(4 * e_host, 1e-12 * hp):
                beyond_host += 1
                assert e_dev <= err, (mu, sigma, r, c1, c2, gap[i], sd0[i], host, hp, err)
    print('normal branch: %d edges, %d with near ties (%d tie nodes), worst sd0 error / host error %.3g, %d beyond 4x the '
          'host (within the fp64 bound)' % (edges_seen, tie_edges, ties, worst_ratio, beyond_host))
    # (an edge whose whole spanning window lies beyond 8 sigma has g below the rounding of 1 + erf: every comparison of its
    # bisection is a near tie, for the host as for the device, and its admissible set is the interval it bisects)
    assert edges_seen > 300
    assert tie_edges <= edges_seen // 100 + 1


# ---- log-normal branch --------------------------------------------------------------------------------------------
def lognormal_edges(seed):
    pmf = H.lognormal_pmf(MU, SIGMA)
    rng = np.random.default_rng(seed)
    spec = [(n, None) for n in range(1, 34)]                                   # every lanes-per-gap width
    spec += [(int(rng.integers(34, 1025)), None) for _ in range(40)]          # small kernel
    spec += [(int(rng.integers(1025, 16385)), None) for _ in range(6)]        # large kernel, observations in LDS
    spec += [(16384, None), (16385, None), (20000, 'far'), (17000, None)]     # observations read from the columns
    spec += [(int(rng.integers(5, 3000)), 'far') for _ in range(24)]          # true gaps near the end of the support
    out = []
    for n, where in spec:
        while True:
            c1, c2 = (int(v) for v in rng.integers(1200, 8000, 2))
            top = pmf.x_max - c1 - c2
            d = int(rng.integers(max(-300, top - 3000), top)) if where == 'far' else int(rng.integers(-300, top))
            e = H.sample_lognormal_edge(rng, pmf, n, d, c1, c2, R)
            if e is not None:
                out.append((e[0], e[1], c1, c2, d))
                break
    rng2 = np.random.default_rng(seed + 1)
    out.append((np.array([150, 160, 170]), np.array([150, 160, 170]), 40, 40, 0))             # every g = 0 (c < r)
    lo = rng2.integers(100, 300, 50)
    out.append((lo, rng2.integers(100, 300, 50), 90, 5000, 0))                                  # c_min <= r
    out.append((np.array([200, 30000]), np.array([200, 300]), 5000, 40000, 0))                 # d_hi < d_lo
    out.append((np.array([0, 1]), np.array([1, pmf.x_max - 1]), 5000, 5000, 0))                # d_lo == d_hi == 0
    return out


def test_lognormal_branch_gap_admissible():
    edges = lognormal_edges(51)
    gb = builder([(lo, hi) for lo, hi, _, _, _ in edges])
    m = len(edges)
    len1 = np.array([e[2] for e in edges], np.int32)
    len2 = np.array([e[3] for e in edges], np.int32)
    x_max = MC.lognormal_support(MU, SIGMA)
    rows = np.arange(m, dtype=np.uint32)
    gap, sd0, _, flags = gb.score_edges(rows, np.zeros(m, np.uint8), len1, len2, 3000.0, 10.0, R,
                                        lognormal=(MU, SIGMA, x_max, 10 ** 6))
    ties = host_moved = 0
    far = []
    for i, (lo, hi, c1, c2, d) in enumerate(edges):
        obs = (np.asarray(lo, np.int64) + np.asarray(hi, np.int64))
        assert flags[i] & 1
        adm, t = H.lognormal_gap(MU, SIGMA, R, obs, c1, c2)
        ties += t
        assert int(gap[i]) in adm, (i, len(obs), c1, c2, d, gap[i], sorted(adm))
        host = MC.lognormal_GapEstimator(MU, SIGMA, R, obs, c1, c2)
        assert host in adm, (i, len(obs), c1, c2, d, host, sorted(adm))
        host_moved += int(gap[i]) != host
        if int(gap[i]) > 12000:
            far.append(int(gap[i]))
    print('log-normal branch: %d edges, %d near ties, %d device != host, %d gaps beyond 12 kb (largest %d of x_max %d)' % (
        m, ties, host_moved, len(far), max(far or [0]), x_max))
    assert len(far) >= 10 and max(far) > 20000
    assert ties <= m // 50 + 1
    assert np.all(sd0 == 2.0 ** 32)
    # the clamp of CreateGraph.py:527-528 on the same edges
    clamp = 5000
    gap_c, _, _, _ = gb.score_edges(rows, np.zeros(m, np.uint8), len1, len2, 3000.0, 10.0, R,
                                    lognormal=(MU, SIGMA, x_max, clamp))
    assert np.array_equal(gap_c, np.minimum(gap, float(clamp)))


# ---- gap table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mu,sigma,r', [(500.0, 50.0, 100), (2500.0, 250.0, 100.38)])
def test_gap_table_rounds_like_the_mpmath_condition(mu, sigma, r):
    from besst_amd import device
    big = 10.0 * (mu + 4 * sigma) + 10.0 * r
    d_lower, d_upper = int(-2 * sigma), int(mu + 2 * sigma - 2 * r)
    with device.GraphContext(0) as ctx:
        vals = ctx.gap_condition_table(mu, sigma, r, big, d_lower, d_upper - d_lower + 1)
    near = 0
    for k, v in enumerate(vals):
        f, err = H.ml_condition(float(d_lower + k), mu, sigma, big, big, r)
        want = math.floor(float(f) + 0.5)
        if math.floor(v + 0.5) != want:
            boundary = want + 0.5 if v > float(f) else want - 0.5
            assert abs(float(f) - boundary) <= H.NORMAL_TOL * err, (d_lower + k, v, float(f), err)
            near += 1
        assert abs(v - float(f)) <= err, (d_lower + k, v, float(f), err)
    assert near <= len(vals) // 100 + 1
