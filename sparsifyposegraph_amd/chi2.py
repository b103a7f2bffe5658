"""The chi^2 quantiles detectOutliers(significance=p) and compatibleCandidates(significance=p) turn into thresholds, in pure
Python (no scipy)."""
import math


def chi2_quantile(q, dof):
    """The q-quantile of chi^2 with `dof` degrees of freedom, in pure Python: bisection on the regularised lower incomplete
    gamma function P(dof / 2, x / 2), by its series below a + 1 and Lentz's continued fraction above (both converge to
    rounding), 200 halvings of a bracket that is doubled until it holds q."""
    if not (0.0 < q < 1.0) or dof <= 0:
        raise ValueError("chi2_quantile: q must lie in (0, 1) and dof be positive")
    a = 0.5 * dof

    def P(x):
        if x <= 0.0:
            return 0.0
        lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
        if x < a + 1.0:
            term = total = 1.0 / a
            n = a
            for _ in range(10000):
                n += 1.0
                term *= x / n
                total += term
                if abs(term) < abs(total) * 1e-17:
                    break
            return total * lead
        tiny = 1e-300
        b = x + 1.0 - a
        c, d = 1.0 / tiny, 1.0 / b
        h = d
        for i in range(1, 10000):
            an = -i * (i - a)
            b += 2.0
            d = an * d + b
            d = tiny if abs(d) < tiny else d
            c = b + an / c
            c = tiny if abs(c) < tiny else c
            d = 1.0 / d
            delta = d * c
            h *= delta
            if abs(delta - 1.0) < 1e-16:
                break
        return 1.0 - lead * h

    lo, hi = 0.0, max(2.0 * a, 1.0)
    while P(0.5 * hi) < q:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if P(0.5 * mid) < q:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _lower_gamma_P(a, x):
    """The regularised lower incomplete gamma function P(a, x): its series below a + 1, Lentz's continued fraction above."""
    if x <= 0.0:
        return 0.0
    lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1.0:
        term = total = 1.0 / a
        n = a
        for _ in range(100000):
            n += 1.0
            term *= x / n
            total += term
            if abs(term) < abs(total) * 1e-17:
                break
        return total * lead
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return 1.0 - lead * h


def chi2_quantile_table(q, dof_step, count):
    """The q-quantiles of chi^2 with dof_step, 2 dof_step, ..., count dof_step degrees of freedom (the joint gate of
    compatibleCandidates: D, 2D, ... for sets of 1, 2, ... candidates). The quantile grows with the degrees of freedom, and
    by less than dof_step + a few standard deviations per entry, so each entry is bisected in a bracket that starts at the
    previous one: [previous, previous + dof_step + 8 sqrt(2 dof)], widened if it does not hold q, 80 halvings."""
    if not (0.0 < q < 1.0) or dof_step <= 0 or count < 0:
        raise ValueError("chi2_quantile_table: q must lie in (0, 1), dof_step be positive and count not negative")
    out, prev = [], 0.0
    for p in range(1, count + 1):
        dof = p * dof_step
        a = 0.5 * dof
        lo, hi = prev, prev + dof_step + 8.0 * math.sqrt(2.0 * dof)
        while _lower_gamma_P(a, 0.5 * hi) < q:
            hi += hi - lo
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            if _lower_gamma_P(a, 0.5 * mid) < q:
                lo = mid
            else:
                hi = mid
        prev = 0.5 * (lo + hi)
        out.append(prev)
    return out
