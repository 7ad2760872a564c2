"""High-precision references for the per-edge numbers of score_kernel (besst_amd/csrc/score.hip) - test infrastructure.

The device kernel and the host restatement (besst_amd/mathstats_compat.py) evaluate the same model in fp64 with different
erf / exp / log and different summation orders, so neither can serve as the other's reference where the last bits decide:
a bisection step whose condition lies within rounding of the naive gap, two gaps of a log-normal scan whose likelihoods
tie to a few ulps.  This module evaluates the same operations far more precisely (mpmath at 40 digits for the normal
branch, 80-bit long doubles for the log-normal likelihood) and, where a decision lies within fp64 rounding of the
boundary (a NEAR TIE), follows both branches.  The result is the set of ADMISSIBLE outputs: any fp64 evaluation that
is accurate to the stated tolerance lands in it, and an output outside it is a bug.

  normal_gap(...)       -> (admissible gaps, near ties met): the bisection of mathstats_compat.GapEstimator replayed
                           node by node (fp64 bracket ends and midpoints, the ML condition in mpmath).
  sk_std_dev(...)       -> (tr_sk_std_dev of the same closed form in mpmath, a bound on its fp64 evaluation error).
  ml_condition(...)     -> (d + sigma^2 g'(d) / g(d) in mpmath, a bound on its fp64 evaluation error).
  lognormal_gap(...)    -> (admissible gaps, near ties met): the two-stage scan of mathstats_compat.lognormal_GapEstimator
                           over L(d) = sum_i log f(o_i + d) - n log g(d), the log terms summed directly and g(d) as a
                           direct weighted sum of the pmf over the support (no prefix differences), both in long double.
  ks_lists(...)         -> the centred lists py_oracle.score_edges hands to py_oracle.ks_h (the specification of h: the
                           reference compares Python floats).
"""
import math

import mpmath
import numpy as np

DPS = 40
EPS = 2.0 ** -52                         # fp64 unit roundoff x 2
NORMAL_TOL = 16.0                        # near tie: |f(mid) - naive| <= NORMAL_TOL x the fp64 error bound of f(mid)
LN_TOL = 2.0 ** -44                      # near tie in the log-normal scan: within LN_TOL x sum of |terms| of L(d)

LONG_DOUBLE_OK = np.finfo(np.longdouble).nmant >= 63


# ---- normal branch ------------------------------------------------------------------------------------------------
def _pieces(d, mean, sigma, c_min, c_max, r):
    lo1 = d + 2 * r - 1 - mean
    hi1 = d + c_min + r - mean
    lo3 = d + c_max + r - mean
    hi3 = d + c_min + c_max + 1 - mean
    return (lo1, hi1, lo3, hi3), ((lo1, hi1, 1, -lo1), (hi1, lo3, 0, c_min - r + 1), (lo3, hi3, -1, hi3))


def _moments(d, mean, sigma, c_min, c_max, r, kmax):
    """(M_0..M_kmax, g'(d), error bounds of the fp64 M_k, error bound of the fp64 g') - the closed form of
    mathstats_compat._weighted_moments in mpmath; the bounds model an fp64 evaluation whose erf / exp are faithful and whose
    breakpoints carry their own rounding (EPS x the size of the terms they are formed from)."""
    mp = mpmath.mp
    with mpmath.workdps(DPS):
        d, mean, sigma, c_min, c_max, r = (mpmath.mpf(v) for v in (d, mean, sigma, c_min, c_max, r))
        s2 = sigma * sigma
        inv = 1 / (mpmath.sqrt(2 * mp.pi) * sigma)
        sq2s = mpmath.sqrt(2) * sigma
        bp, pieces = _pieces(d, mean, sigma, c_min, c_max, r)
        e_bp = EPS * (abs(d) + abs(mean) + c_min + c_max + 2 * abs(r) + 1)      # rounding of a breakpoint
        Phi, p, ePhi, ep = {}, {}, {}, {}
        for y in bp:
            if y in Phi:
                continue
            Phi[y] = (1 + mpmath.erf(y / sq2s)) / 2
            p[y] = inv * mpmath.exp(-(y * y) / (2 * s2))
            ePhi[y] = EPS + p[y] * e_bp
            ep[y] = p[y] * (4 * EPS + 2 * EPS * y * y / s2 + abs(y) * e_bp / s2)
        M = [mpmath.mpf(0)] * (kmax + 1)
        eM = [mpmath.mpf(0)] * (kmax + 1)
        for a, b, alpha, beta in pieces:
            if not (b > a):
                continue
            B = [Phi[b] - Phi[a], -s2 * (p[b] - p[a])]
            eB = [ePhi[a] + ePhi[b] + EPS * abs(B[0]), s2 * (ep[a] + ep[b]) + EPS * abs(B[1])]
            for k in range(2, kmax + 2):
                B.append((k - 1) * s2 * B[k - 2] - s2 * (b ** (k - 1) * p[b] - a ** (k - 1) * p[a]))
                eB.append((k - 1) * s2 * eB[k - 2] + s2 * (abs(b) ** (k - 1) * ep[b] + abs(a) ** (k - 1) * ep[a]
                                                         + (k - 1) * (abs(b) ** (k - 2) * p[b] + abs(a) ** (k - 2) * p[a]) * e_bp)
                          + 2 * EPS * ((k - 1) * s2 * abs(B[k - 2]) + s2 * (abs(b) ** (k - 1) * p[b] + abs(a) ** (k - 1) * p[a])))
            for k in range(kmax + 1):
                M[k] += alpha * B[k + 1] + beta * B[k]
                eM[k] += abs(alpha) * eB[k + 1] + (abs(beta) + e_bp) * eB[k] + 2 * EPS * (abs(alpha * B[k + 1]) + abs(beta * B[k]))
        eg = eM[0]
        lo1, hi1, lo3, hi3 = bp
        gp = mpmath.mpf(0)
        egp = mpmath.mpf(0)
        if hi3 > lo3:
            gp += Phi[hi3] - Phi[lo3]
            egp += ePhi[hi3] + ePhi[lo3]
        if hi1 > lo1:
            gp -= Phi[hi1] - Phi[lo1]
            egp += ePhi[hi1] + ePhi[lo1]
        return M, gp, eM, egp


def ml_condition(d, mean, sigma, c_min, c_max, r):
    """(f, err): f = d + sigma^2 g'(d) / g(d) (d where g <= 0, as the restatement), err a bound on |fp64 f - f|; err is
    inf where g is not above its own fp64 error (an fp64 evaluation may then take either branch of `g > 0`)."""
    M, gp, eM, egp = _moments(d, mean, sigma, c_min, c_max, r, 0)
    g, eg = M[0], eM[0]
    with mpmath.workdps(DPS):
        if g > 0 and g > 4 * eg:
            s2 = mpmath.mpf(sigma) ** 2
            f = d + s2 * gp / g
            err = s2 * (egp / g + abs(gp) * eg / (g * g)) + EPS * (abs(d) + abs(f - d))
            return f, float(err)
        if g == 0 and eg == 0:
            return mpmath.mpf(d), 0.0                        # no piece at all: f = d exactly
        if g <= 0 and -g > 4 * eg:
            return mpmath.mpf(d), 0.0                        # g < 0 beyond doubt: f = d as in fp64
        return mpmath.mpf(d), math.inf


class _Condition(object):
    """ml_condition of one parameter set, memoised over the bisection nodes (edges of one parameter set share them)."""

    def __init__(self, mean, sigma, r, c1, c2):
        self.args = (float(mean), float(sigma), float(min(c1, c2)), float(max(c1, c2)), float(r))
        self.memo = {}

    def __call__(self, d):
        v = self.memo.get(d)
        if v is None:
            mean, sigma, c_min, c_max, r = self.args
            v = self.memo[d] = ml_condition(d, mean, sigma, c_min, c_max, r)
        return v


_COND_CACHE = {}


def _condition(mean, sigma, r, c1, c2):
    key = (float(mean), float(sigma), float(r), float(min(c1, c2)), float(max(c1, c2)))
    c = _COND_CACHE.get(key)
    if c is None:
        if len(_COND_CACHE) > 512:
            _COND_CACHE.clear()
        c = _COND_CACHE[key] = _Condition(mean, sigma, r, c1, c2)
    return c


def normal_gap(mean, sigma, read_len, mean_obs, c1, c2, tol=NORMAL_TOL):
    """Admissible results of GapEstimator(mean, sigma, read_len, mean_obs, c1, c2) -> (set of gaps, near ties met).
    naive = mean - mean_obs in fp64; bracket ends trunc() in fp64 and (hi + lo) / 2.0 midpoints, exactly as the host and
    the device form them; each comparison f(mid) > naive decided in mpmath unless it is within tol x the fp64 error bound
    of f(mid), where both branches are followed."""
    cond = _condition(mean, sigma, read_len, c1, c2)
    naive = float(mean) - float(mean_obs)
    upper = float(int(mean + 4 * sigma - 2 * read_len))
    lower = float(int(-4 * sigma))
    out, ties = set(), 0
    stack = [(lower, upper)]
    while stack:
        lo, hi = stack.pop()
        if not (hi - lo > 1):
            out.add(int(math.floor((hi + lo) / 2.0 + 0.5)))
            continue
        mid = (hi + lo) / 2.0
        f, err = cond(mid)
        with mpmath.workdps(DPS):
            delta = f - mpmath.mpf(naive)
        if abs(delta) <= tol * err:
            ties += 1
            stack.append((lo, mid))
            stack.append((mid, hi))
        elif delta > 0:
            stack.append((lo, mid))
        else:
            stack.append((mid, hi))
    return out, ties


def sk_std_dev(mean, sigma, read_len, c1, c2, d):
    """(sigma, err): tr_sk_std_dev of the closed form in mpmath (2**32 where M_0 <= 0, 0 where the variance is not
    positive) and a bound on the error of an fp64 evaluation of it (inf where the sign of M_0 or of the variance is within
    rounding).  Near the ends of the bracket the variance is a difference of nearly equal terms: the bound is then far
    above 1e-12 relative, for the host as for the device."""
    M, _, eM, _ = _moments(float(d), mean, sigma, float(min(c1, c2)), float(max(c1, c2)), read_len, 2)
    with mpmath.workdps(DPS):
        if not (M[0] > 4 * eM[0]):
            return float(2 ** 32), (0.0 if M[0] <= 0 and -M[0] > 4 * eM[0] or M[0] == eM[0] == 0 else math.inf)
        e1 = M[1] / M[0]
        var = M[2] / M[0] - e1 * e1
        e_e1 = eM[1] / M[0] + abs(M[1]) * eM[0] / M[0] ** 2
        e_var = eM[2] / M[0] + abs(M[2]) * eM[0] / M[0] ** 2 + 2 * abs(e1) * e_e1 + 2 * EPS * (abs(M[2] / M[0]) + e1 * e1)
        if not (var > 4 * e_var):
            return (float(mpmath.sqrt(var)) if var > 0 else 0.0), math.inf
        sd = mpmath.sqrt(var)
        return float(sd), float(e_var / (2 * sd) + EPS * sd)


# ---- log-normal branch --------------------------------------------------------------------------------------------
class LogNormalPmf(object):
    """The pmf f(x), x = 1 .. x_max, of the log-normal library (mathstats_compat.lognormal_support), in long double
    (mpmath where long double is not the 80-bit format)."""

    def __init__(self, mu, sigma):
        from besst_amd import mathstats_compat as MC
        self.mu, self.sigma = float(mu), float(sigma)
        self.x_max = MC.lognormal_support(mu, sigma)
        if LONG_DOUBLE_OK:
            x = np.arange(1, self.x_max + 1).astype(np.longdouble)
            lx = np.log(x)
            mu_l, s_l = np.longdouble(self.mu), np.longdouble(self.sigma)
            self.f = np.exp(-((lx - mu_l) ** 2) / (2 * s_l * s_l)) / (x * s_l * np.sqrt(2 * np.longdouble(math.pi)))
        else:
            with mpmath.workdps(30):
                self.f = [self._f_mp(x) for x in range(1, self.x_max + 1)]

    def _f_mp(self, x):
        lx = mpmath.log(x)
        return mpmath.exp(-((lx - self.mu) ** 2) / (2 * self.sigma ** 2)) / (x * self.sigma * mpmath.sqrt(2 * mpmath.pi))

    def weights(self, d, c_min, c_max, r):
        """(first x, w(x; d) for the x of the window) - the three linear pieces of mathstats_compat._lognormal_log_g,
        placed on the integers and clipped to the support (negative where c_min < r - 1, as the restatement's)."""
        a, b = max(1, d + 2 * r), min(self.x_max, d + c_min + c_max)
        if b < a:
            return a, np.zeros(0, np.int64)
        x = np.arange(a, b + 1, dtype=np.int64)
        w = np.where(x <= d + c_min + r - 1, x - d - 2 * r + 1,
                     np.where(x <= d + c_max + r, c_min - r + 1, c_min + c_max + d - x + 1))
        return a, w

    def g(self, d, c_min, c_max, r):
        """g(d) = sum_x w(x; d) f(x), summed directly over the window."""
        a, w = self.weights(int(d), int(c_min), int(c_max), int(r))
        if w.shape[0] == 0:
            return 0
        if LONG_DOUBLE_OK:
            return np.dot(w.astype(np.longdouble), self.f[a - 1:a - 1 + w.shape[0]])
        with mpmath.workdps(30):
            return mpmath.fsum(int(wi) * fi for wi, fi in zip(w, self.f[a - 1:a - 1 + w.shape[0]]))

    def log_g(self, d, c_min, c_max, r):
        g = self.g(d, c_min, c_max, r)
        if not g > 0:
            return -math.inf
        return np.log(g) if LONG_DOUBLE_OK else mpmath.log(g)


_PMF = {}


def lognormal_pmf(mu, sigma):
    key = (float(mu), float(sigma))
    if key not in _PMF:
        _PMF.clear()
        _PMF[key] = LogNormalPmf(mu, sigma)
    return _PMF[key]


def _loglik(pmf, vals, cnts, ds, c_min, c_max, r):
    """(L(d), sum of |terms| of L(d)) for the gaps ds: vals / cnts the distinct observations and their multiplicities.
    L(d) = -sum_i [log x_i + (log x_i - mu)^2 / (2 sigma^2)] - n log g(d), x_i = o_i + d (the constant n log(sigma
    sqrt(2 pi)) dropped, as the host and the device drop it)."""
    n = int(cnts.sum())
    L = np.empty(len(ds), dtype=object)
    S = np.empty(len(ds), dtype=np.float64)
    for k, d in enumerate(ds):
        lg = pmf.log_g(int(d), c_min, c_max, r)
        if lg == -math.inf:
            L[k], S[k] = -math.inf, 0.0
            continue
        if LONG_DOUBLE_OK:
            lx = np.log((vals + int(d)).astype(np.longdouble))
            t = lx + (lx - np.longdouble(pmf.mu)) ** 2 / (2 * np.longdouble(pmf.sigma) ** 2)
            L[k] = -np.dot(cnts.astype(np.longdouble), t) - n * lg
            S[k] = float(np.dot(cnts.astype(np.longdouble), np.abs(t)) + n * abs(lg))
        else:
            with mpmath.workdps(30):
                ts = [mpmath.log(int(v) + int(d)) for v in vals]
                ts = [t + (t - pmf.mu) ** 2 / (2 * pmf.sigma ** 2) for t in ts]
                L[k] = -mpmath.fsum(int(c) * t for c, t in zip(cnts, ts)) - n * lg
                S[k] = float(mpmath.fsum(int(c) * abs(t) for c, t in zip(cnts, ts)) + n * abs(lg))
    return L, S


def _argmax_set(ds, L, S, tol):
    """The gaps an fp64 argmax (earliest on a tie) can return: those whose L is within the rounding of the best, and
    (-inf everywhere) the first gap.  -> (set, near tie met)."""
    finite = [k for k in range(len(ds)) if L[k] != -math.inf]
    if not finite:
        return {int(ds[0])}, False
    best = max(finite, key=lambda k: (L[k], -k))
    out = set()
    for k in finite:
        if float(L[best] - L[k]) <= tol * (S[best] + S[k]):
            out.add(int(ds[k]))
    # a gap with g within rounding of 0 may be -inf in fp64 or finite: such gaps are never near the argmax in practice
    return out, len(out) > 1


def lognormal_gap(mu, sigma, read_len, samples, c1, c2, tol=LN_TOL):
    """Admissible results of mathstats_compat.lognormal_GapEstimator (and of the device's lognormal_gap) ->
    (set of gaps, near ties met).  Coarse scan with stride 64 from d_lo, then the gaps within 64 of the coarse optimum
    clipped to [d_lo, d_hi]; every coarse gap that is a near tie of the coarse optimum opens its own window.  The
    d_hi < d_lo fall-back is the restatement's int(round(exp(mu) - mean(obs)))."""
    obs = np.asarray(samples, dtype=np.int64)
    pmf = lognormal_pmf(mu, sigma)
    r = int(round(read_len))
    c_min, c_max = int(min(c1, c2)), int(max(c1, c2))
    d_lo, d_hi = 1 - int(obs.min()), pmf.x_max - int(obs.max())
    if d_hi < d_lo:
        return {int(round(math.exp(mu) - float(obs.mean())))}, 0
    vals, cnts = np.unique(obs, return_counts=True)
    coarse = np.arange(d_lo, d_hi + 1, 64, dtype=np.int64)
    L, S = _loglik(pmf, vals, cnts, coarse, c_min, c_max, r)
    centres, tie = _argmax_set(coarse, L, S, tol)
    ties = int(tie)
    out = set()
    for best in sorted(centres):
        fine = np.arange(max(d_lo, best - 64), min(d_hi, best + 64) + 1, dtype=np.int64)
        Lf, Sf = _loglik(pmf, vals, cnts, fine, c_min, c_max, r)
        got, tie = _argmax_set(fine, Lf, Sf, tol)
        ties += int(tie)
        out |= got
    return out, ties


# ---- KS numerator -------------------------------------------------------------------------------------------------
def ks_lists(obs_lo, obs_hi, swap):
    """(l1, l2) as py_oracle.score_edges forms them (py_oracle.py:961-972) from an edge's observation columns: l1 the
    observations on the edge's first endpoint (obs_hi where swap is set), sorted and centred on their mean; l2 the
    distances of the other endpoint's observations from their maximum, ascending, centred - both lists of Python floats."""
    from oracle import py_oracle as O
    a, b = (obs_hi, obs_lo) if swap else (obs_lo, obs_hi)
    l1 = sorted(int(v) for v in a)
    n = len(l1)
    m1 = O._fsum_lr(l1) / float(n)
    l1 = [x - m1 for x in l1]
    l2 = [int(v) for v in b]
    mx = max(l2)
    l2 = [abs(x - mx) for x in sorted(l2, reverse=True)]
    m2 = O._fsum_lr(l2) / float(n)
    return l1, [x - m2 for x in l2]


def ks_h(obs_lo, obs_hi, swap):
    from oracle import py_oracle as O
    return O.ks_h(*ks_lists(obs_lo, obs_hi, swap))


# ---- edges drawn from the log-normal model ------------------------------------------------------------------------
def sample_lognormal_edge(rng, pmf, n, d, c1, c2, r):
    """n links of fragments x ~ f that span a gap d between contigs of lengths c1, c2 with both reads of length r inside
    their contigs -> (obs_lo, obs_hi) int64 arrays (bases of the fragment on contig 1 / contig 2).  x is drawn from
    f(x) x (number of placements), so any gap up to the end of the support can be sampled; None where no fragment spans."""
    x = np.arange(max(1, d + 2 * r), min(pmf.x_max, d + c1 + c2) + 1, dtype=np.int64)
    o = x - d
    w = np.minimum(c1, o - r) - np.maximum(r, o - c2) + 1
    p = np.where(w > 0, w, 0) * np.asarray(pmf.f[x - 1], dtype=np.float64)
    if x.shape[0] == 0 or not p.sum() > 0:
        return None
    xs = rng.choice(x, size=n, p=p / p.sum())
    o = xs - d
    a_lo, a_hi = np.maximum(r, o - c2), np.minimum(c1, o - r)
    lo = a_lo + (rng.random(n) * (a_hi - a_lo + 1)).astype(np.int64)
    return lo, o - lo
