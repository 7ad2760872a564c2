"""The high-precision references of oracle/score_hp.py against the host restatement (besst_amd/mathstats_compat.py) and the
brute-force model (oracle/gapest_numeric.py): what makes them trustworthy as the yardstick of score_kernel
(tests/test_gpu_score_hp.py).  CPU only.

Tolerances asserted here: the host's gap is in the admissible set of the replayed bisection / scan (exact unless a near
tie was met, and near ties are rare); the host's sigma is within the fp64 error bound of the mpmath value; the hp gap is
within the brute-force model's +-1 bp (+-2 at the ends of the search interval); the prefix-difference log g of the host
keeps 1e-13 near the mode and loses precision towards the end of the support, where the direct sum stays exact and the
prefix + tail tables keep 2e-13."""
import math

import mpmath
import numpy as np
import pytest

from besst_amd import mathstats_compat as MC
from oracle import gapest_numeric as GN
from oracle import score_hp as H
from tests.test_gapest_numeric import GRID

FRACS = (-0.6, -0.2, 0.0, 0.3, 0.7, 1.0)
MU, SIGMA, R = math.log(3000.0), 0.35, 100


def random_grid(seed, count):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        mu = float(rng.uniform(300.0, 6000.0))
        sigma = float(mu * rng.uniform(0.04, 0.25))
        r = float(rng.choice([75.0, 100.0, 100.38, 150.0]))
        c1, c2 = (int(v) for v in rng.integers(int(2 * sigma) + 1, 40000, 2))
        if rng.random() < 0.2:
            c2 = c1
        mean_obs = float(rng.uniform(2 * r - 4 * sigma, mu + 4 * sigma))
        out.append((mu, sigma, r, c1, c2, mean_obs))
    return out


def test_long_double_is_the_80_bit_format():
    # the log-normal references use long double where it has 64 mantissa bits, mpmath otherwise
    assert H.LONG_DOUBLE_OK == (np.finfo(np.longdouble).nmant >= 63)


def test_normal_gap_is_the_host_bisection():
    cases = [(mu, sigma, r, c1, c2, mu - f * (mu - 2 * r)) for mu, sigma, r, c1, c2 in GRID for f in FRACS]
    cases += random_grid(3, 150)
    ties = 0
    for mu, sigma, r, c1, c2, mean_obs in cases:
        got, t = H.normal_gap(mu, sigma, r, mean_obs, c1, c2)
        host = MC.GapEstimator(mu, sigma, r, mean_obs, c1, c2)
        assert host in got, (mu, sigma, r, c1, c2, mean_obs, got, host)
        assert t > 0 or len(got) == 1
        ties += t > 0
    assert ties <= len(cases) // 100 + 1


@pytest.mark.parametrize('mu,sigma,r,c1,c2', GRID)
def test_normal_gap_agrees_with_the_brute_force_model(mu, sigma, r, c1, c2):
    ri = int(round(r))
    lo, hi = int(-4 * sigma), int(mu + 4 * sigma - 2 * r)
    for f in (FRACS if mu < 5000 else (-0.2, 0.7)):        # (the brute force is slow for wide libraries)
        mean_obs = mu - f * (mu - 2 * r)
        got, _ = H.normal_gap(mu, sigma, r, mean_obs, c1, c2)
        want, fs = GN.ml_gap(mu, sigma, ri, mean_obs, c1, c2)
        tol = 2 if want in (lo, hi, min(fs), max(fs)) else 1
        assert all(abs(g - want) <= tol for g in got), (f, got, want)


def test_normal_gap_edges_of_the_bracket():
    # mean_obs outside the bracket pins the gap at an end; a pair of contigs too short for any placement (g = 0: the
    # condition is d itself, the bisection converges on the naive gap)
    mu, sigma, r = 2500.0, 250.0, 100
    lo, hi = int(-4 * sigma), int(mu + 4 * sigma - 2 * r)
    assert H.normal_gap(mu, sigma, r, mu + 10 * sigma, 5000, 8000)[0] == {lo}
    assert H.normal_gap(mu, sigma, r, 1.0, 5000, 8000)[0] == {hi}
    got, t = H.normal_gap(500.0, 10.0, 100, 480.0, 60, 60)
    assert got == {MC.GapEstimator(500.0, 10.0, 100, 480.0, 60, 60)} and t == 0
    assert H.sk_std_dev(500.0, 10.0, 100, 60, 60, 20) == (2.0 ** 32, 0.0)


def test_sigma_is_the_host_sigma():
    worst = 0.0
    for mu, sigma, r, c1, c2 in GRID:
        ri = int(round(r))
        for d in (int(-4 * sigma), int(-2 * sigma), -50, 0, 100, int(mu / 2), int(mu), int(mu + 4 * sigma - 2 * r)):
            want, err = H.sk_std_dev(mu, sigma, r, c1, c2, d)
            host = MC.tr_sk_std_dev(mu, sigma, r, c1, c2, d)
            assert abs(host - want) <= err, (mu, sigma, r, c1, c2, d, host, want, err)
            worst = max(worst, abs(host - want) / want)
            bf = GN.span_sd(d, mu, sigma, c1, c2, ri)
            if bf is not None and want < 2 ** 31 and d in (-50, 0, 100, int(mu / 2)):
                assert abs(want - bf) <= 0.005 * bf + 0.05, (d, want, bf)
    assert worst > 0.0                       # (the host is not the reference: it does round)


def test_ml_condition_is_the_host_condition():
    for mu, sigma, r in ((500.0, 50.0, 100), (5199.56, 499.55, 100), (2500.0, 250.0, 100.38)):
        big = 10.0 * (mu + 4 * sigma) + 10.0 * r
        for d in range(int(-2 * sigma), int(mu + 2 * sigma - 2 * r) + 1, 37):
            want, err = H.ml_condition(float(d), mu, sigma, big, big, r)
            host = MC.ml_condition(float(d), mu, sigma, big, big, r)
            assert abs(host - float(want)) <= err, (d, host, want, err)


def lognormal_edges(seed, count, n_choices, r=R, d_max=None):
    pmf = H.lognormal_pmf(MU, SIGMA)
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        c1, c2 = (int(v) for v in rng.integers(1200, 8000, 2))
        hi = pmf.x_max - c1 - c2 if d_max is None else d_max
        d = int(rng.integers(-300, max(-299, hi)))
        n = int(rng.choice(n_choices))
        e = H.sample_lognormal_edge(rng, pmf, n, d, c1, c2, r)
        if e is not None:
            out.append((d, c1, c2, e[0] + e[1]))
    return out


def test_lognormal_gap_is_the_host_scan():
    """True gaps up to the end of the support (x_max - max(obs)), 1 to 3000 links."""
    moved = ties = 0
    edges = lognormal_edges(5, 40, (1, 2, 5, 33, 400, 3000))
    for d, c1, c2, obs in edges:
        got, t = H.lognormal_gap(MU, SIGMA, R, obs, c1, c2)
        host = MC.lognormal_GapEstimator(MU, SIGMA, R, obs, c1, c2)
        assert host in got, (d, c1, c2, len(obs), sorted(got), host)
        moved += len(got) > 1
        ties += t
    assert max(d for d, _, _, _ in edges) > 15000
    assert ties <= 1 and moved <= 1


def test_lognormal_gap_edge_cases():
    x_max = MC.lognormal_support(MU, SIGMA)
    # observations beyond the support: the fall-back of the restatement
    obs = [200, 25000]
    assert H.lognormal_gap(MU, SIGMA, R, obs, 5000, 30000) == ({MC.lognormal_GapEstimator(MU, SIGMA, R, obs, 5000, 30000)}, 0)
    # no gap with a spanning fragment (contigs shorter than a read: every g is 0): the earliest gap
    obs = [150, 160, 170]
    got, _ = H.lognormal_gap(MU, SIGMA, R, obs, 40, 40)
    assert got == {1 - 150} == {MC.lognormal_GapEstimator(MU, SIGMA, R, obs, 40, 40)}
    # c_min <= r: the middle piece has a non-positive weight
    obs = [230, 260, 300, 410]
    got, _ = H.lognormal_gap(MU, SIGMA, R, obs, 90, 5000)
    assert MC.lognormal_GapEstimator(MU, SIGMA, R, obs, 90, 5000) in got
    # observations at both ends of the support: d_lo == d_hi == 0
    assert H.lognormal_gap(MU, SIGMA, R, [1, x_max], 5000, 5000)[0] == {0} == {MC.lognormal_GapEstimator(
        MU, SIGMA, R, [1, x_max], 5000, 5000)}


def test_direct_g_is_exact_and_the_tables_keep_its_precision():
    """log g(d) against the direct long-double sum (itself within 1e-17 of a 30-digit mpmath sum).  The prefix tables alone
    keep 1e-13 near the mode and lose precision towards the end of the support (4e-5 at 23.6 kb, 4e-3 at 24.3 kb: the
    argmax of the scan moves there, see test_lognormal_gap_is_the_host_scan); with the tail tables above the median the
    host (and the device) keep 2e-13 at every gap, for long and short contigs."""
    pmf = H.lognormal_pmf(MU, SIGMA)
    x_max, F0, F1 = MC._lognormal_tables(MU, SIGMA)
    tails = MC._lognormal_tail_tables(MU, SIGMA)
    for c_min, c_max in ((5000, 7000), (1200, 1500), (300, 400)):
        err, err_prefix = {}, {}
        for d in (-250, -100, 0, 500, 2000, 9600, 15000, 20000, 23600, 24270, x_max - c_min - c_max - 150):
            hp = pmf.log_g(d, c_min, c_max, R)
            if hp == -math.inf:
                continue
            hp = float(hp)
            err[d] = abs(float(MC._lognormal_log_g(np.array([d]), x_max, F0, F1, c_min, c_max, R, tails)[0]) - hp)
            err_prefix[d] = abs(float(MC._lognormal_log_g(np.array([d]), x_max, F0, F1, c_min, c_max, R)[0]) - hp)
        assert max(err.values()) < 2e-13, (c_min, c_max, err)
        assert err_prefix[0] < 1e-13 and err_prefix[23600] > 1e-5 and err_prefix[24270] > 1e-3
    for d in (0, 23600):
        a, w = pmf.weights(d, 5000, 7000, R)
        with mpmath.workdps(30):
            ref = mpmath.log(mpmath.fsum(int(wi) * pmf._f_mp(a + k) for k, wi in enumerate(w)))
            mine = pmf.log_g(d, 5000, 7000, R)
            assert abs(float(ref - mpmath.mpf(str(mine)))) < 1e-17 * max(1.0, abs(float(ref)))


def test_prefix_and_tail_tables():
    """The prefix tables are the plain cumulative sums; the tail tables hold the rest of the mass above K."""
    x_max, F0, F1 = MC._lognormal_tables(MU, SIGMA)
    K, G0, G1 = MC._lognormal_tail_tables(MU, SIGMA)
    assert K == MC._lognormal_split(MU, x_max) == int(math.floor(3000.0 + 0.5))
    assert F0.shape[0] == x_max + 1 and F0[0] == 0.0 and np.all(np.diff(F0) >= 0)
    assert G0.shape[0] == G1.shape[0] == x_max - K + 1 and G0[-1] == 0.0 == G1[-1] and np.all(np.diff(G0) <= 0)
    assert abs(F0[K] + G0[0] - 1.0) < 1e-8                  # all the mass (6 sigma: 1e-9 beyond x_max)
    assert abs(F0[x_max] - F0[K] - G0[0]) < 1e-13 and abs(F1[x_max] - F1[K] - G1[0]) < 1e-13 * F1[x_max]
