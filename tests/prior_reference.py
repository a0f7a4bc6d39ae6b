"""A plain float64 statement of the element-wise priors of the HIP prior hook (kinds 1-9 of include/sgmcmc_hip.h,
SURVEY.md Appendix A) with the rounding-error budget of each family next to its formula, and of its two whitened kinds
(10 and 11: ``whitened``).

Independent of ``bnn_priors_amd.prior``: numpy plus ``math.lgamma`` / ``math.erfc`` / ``math.log1p``.  Inputs are the
values AS STORED (an fp32 arena's theta, g and raw hyper-parameter s widened exactly); ``loc``, ``scale``, ``df`` and ``N``
are the doubles of the segment table.

The budgets restate what csrc/sgmcmc_hip.hip documents -- "the gradient is applied in the working precision with one
rounding for the factor and one fma into g; log p is evaluated and accumulated in fp64" -- with u the unit roundoff of the
working precision T (2^-24 / 2^-53), first order in u, and ONE safety factor of 2 (``SAFETY``) for the second-order terms.
To every bound the reference's own float64 rounding is added (``U64`` times the operations this file performs on the term,
stated where it is added): it is negligible against an fp32 budget and is what keeps an fp64 comparison honest.
"""
import math

import numpy as np

NONE, NORMAL, LAPLACE, STUDENT_T, CAUCHY, GENNORM = 0, 1, 2, 3, 4, 5
GAMMA_SOFTPLUS, UNIFORM_CDF, HALFCAUCHY_SOFTPLUS, IMPROPER_SOFTPLUS = 6, 7, 8, 9
HYPER_KINDS = (GAMMA_SOFTPLUS, UNIFORM_CDF, HALFCAUCHY_SOFTPLUS, IMPROPER_SOFTPLUS)
FILTER_WHITENED, MULTIVARIATE_T = 10, 11
BASE_NORMAL, BASE_GENNORM, BASE_LAPLACE, BASE_DOUBLE_GAMMA = 0, 1, 2, 3

U32, U64 = 2.0 ** -24, 2.0 ** -53
SAFETY = 2.0
SUBNORMAL = {U32: 2.0 ** -149, U64: 2.0 ** -1074}     # absolute error of a result that underflows gradually
LARGEST = {U32: float(np.finfo(np.float32).max), U64: float(np.finfo(np.float64).max)}
# the log-density: "fp64 evaluation of the stored values": numel * 2^-50 RELATIVE (8 roundings per accumulated element)
LOGP_REL_PER_ELEMENT = 2.0 ** -50
_quiet = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


def unit_roundoff(dtype_name):
    return {"float32": U32, "float64": U64}[dtype_name]


def fround(x, u):
    "x rounded to the working precision (a python float again)"
    return float(np.float32(x)) if u == U32 else float(x)


# --------------------------------------------------------------------------------------------------- hyper segments
def softplus(s):
    "log(1 + e^s) without the cut-off the kernel (s > 30) or torch (s > 20) take"
    return s + math.log1p(math.exp(-s)) if s > 0 else math.log1p(math.exp(s))


def sigmoid(s):
    if s >= 0:
        return 1.0 / (1.0 + math.exp(-s))
    e = math.exp(s)
    return e / (1.0 + e)


def hyper_value(kind, loc, scale, s):
    """(x, dx/ds, rel): the value of a hierarchical scale at raw parameter s, its derivative, and the RELATIVE allowance on
    x as the kernel forms it in fp64: 8 roundings (exp, log1p / erfc, the products), plus -- GAMMA / HALFCAUCHY / IMPROPER
    beyond s = 30 -- the documented cut ``s > 30 ? s : log1p(exp(s))``, which drops log1p(e^-s) <= e^-30 = 9.4e-14
    (1.9e-15 relative at s = 30.5: 17 units of 2^-53, which an fp64 arena sees)."""
    if kind == UNIFORM_CDF:                   # low = loc, high = scale
        w = scale - loc
        x = loc + w * 0.5 * math.erfc(-s * math.sqrt(0.5))
        return x, w * math.exp(-0.5 * s * s) / math.sqrt(2.0 * math.pi), 8 * U64
    sp, sig = softplus(s), sigmoid(s)
    rel = 8 * U64 + (math.log1p(math.exp(-s)) / sp if s > 30.0 else 0.0)
    if kind == HALFCAUCHY_SOFTPLUS:           # loc = multiplier
        return sp * loc, sig * loc, rel
    assert kind in (GAMMA_SOFTPLUS, IMPROPER_SOFTPLUS), kind
    return sp, sig, rel


def hyper_log_density(kind, loc, scale, s):
    """(log p, d log p / ds, |.|-sum of the derivative's terms) of a hyper-prior kind at raw parameter s; the density is
    that of the VALUE without a Jacobian (prior/transformed.py)"""
    if kind == IMPROPER_SOFTPLUS:
        return 0.0, 0.0, 0.0
    if kind == UNIFORM_CDF:
        return -math.log(scale - loc), 0.0, 0.0
    sp, sig = softplus(s), sigmoid(s)
    if kind == GAMMA_SOFTPLUS:                # loc = concentration c, scale = rate r
        lp = loc * math.log(scale) - math.lgamma(loc) + (loc - 1.0) * math.log(sp) - scale * sp
        return lp, ((loc - 1.0) / sp - scale) * sig, (abs(loc - 1.0) / sp + abs(scale)) * sig
    assert kind == HALFCAUCHY_SOFTPLUS, kind   # loc = multiplier, scale = gamma
    z = sp * loc / scale
    lp = math.log(2.0 / (math.pi * scale)) - math.log1p(z * z)
    d = -2.0 * z / (1.0 + z * z) * (loc / scale) * sig
    return lp, d, abs(d)


def hyper_segment(kind, loc, scale, s, N, g_h, u, chains=()):
    """The hyper segment's gradient after sgmcmc_prior_grad: g_h - (1/N)(d log p_hyper / ds + sum over the linked weight
    segments of D dx/ds), D = sum_j d log p(theta_j) / d scale (``elementwise(...)["dls"]``).  ``chains`` holds one
    ``elementwise`` result per linked weight segment.

    Budget.  "Hyper kinds: two roundings in T": the prior kernel rounds g_h - dlp / N into T, hyper_link_kernel then rounds
    that minus the chain-rule term into T: u (|a| + |g'|) with a the intermediate.  The own term is fp64 arithmetic of
    ~16 operations on its |.|-sum.  Chain-rule sum: numel * 2^-53 * sum|d log p / d scale| * |dx/ds| / N for the fp64
    accumulation over elements and chunks in any order, 8 more roundings for each element's own evaluation and dx/ds, and
    the scale's allowance (d dls / d ln scale <= 3 |dls|-sum)."""
    x, dxds, rel = hyper_value(kind, loc, scale, s)
    lp, dlp, dlp_abs = hyper_log_density(kind, loc, scale, s)
    a = g_h - dlp / N
    out, budget = a, u * abs(a) + rel * dlp_abs / N       # (the own term moves with x by no more than its |.|-sum)
    for w in chains:
        chain = w["dls"] * dxds / N
        out -= chain
        budget += ((w["numel"] + 8) * U64 + 3 * rel) * w["dls_abs"] * abs(dxds) / N
    budget += u * abs(out)
    ref_own = U64 * (16 * dlp_abs / N + 2 * abs(a) + 2 * abs(out))
    # the log-density: ~32 fp64 operations on the |.|-sum of its terms, and x's allowance through d log p / d log x
    # (GAMMA: (c - 1) - r x; HALFCAUCHY: -2 z^2 / (1 + z^2))
    slope = {GAMMA_SOFTPLUS: abs(loc - 1.0) + abs(scale) * x, HALFCAUCHY_SOFTPLUS: 2.0}.get(kind, 0.0)
    return dict(x=x, dxds=dxds, x_rel=rel, g=out, bound=SAFETY * budget + ref_own, logp=lp,
                logp_bound=32 * U64 * (abs(lp) + _hyper_logp_abs(kind, loc, scale, s)) + rel * slope)


def _hyper_logp_abs(kind, loc, scale, s):
    "|.|-sum of the hyper log-density's terms (they cancel: c log r - lgamma(c) + (c - 1) log x - r x)"
    if kind == GAMMA_SOFTPLUS:
        sp = softplus(s)
        return abs(loc * math.log(scale)) + abs(math.lgamma(loc)) + abs((loc - 1.0) * math.log(sp)) + abs(scale * sp)
    if kind == HALFCAUCHY_SOFTPLUS:
        z = softplus(s) * loc / scale
        return abs(math.log(2.0 / (math.pi * scale))) + math.log1p(z * z)
    return 0.0


# --------------------------------------------------------------------------------------------------- weight segments
def lgamma_half_step(a):
    """lgamma(a + 1/2) - lgamma(a).  From a = 32 on by Stirling's series subtracted term by term (either lgamma is ~a log a
    there, and math.lgamma's last bit of it would be all that is left of a normaliser of order 1: 5e-10 at a = 5e5);
    first omitted term < 4e-18."""
    if a < 32.0:
        return math.lgamma(a + 0.5) - math.lgamma(a)
    b = a + 0.5
    series = sum(c * (b ** -k - a ** -k) for k, c in ((1, 1 / 12.), (3, -1 / 360.), (5, 1 / 1260.), (7, -1 / 1680.)))
    return a * math.log1p(0.5 / a) + 0.5 * (math.log(a) - 1.0) + series


def log_norm_terms(kind, scale, df):
    "the terms of the normalising constant of ONE element's log-density (they cancel: their |.|-sum sizes its rounding)"
    if kind == NORMAL:
        return [-math.log(scale), -0.5 * math.log(2.0 * math.pi)]
    if kind == LAPLACE:
        return [-math.log(2.0 * scale)]
    if kind == STUDENT_T:
        a = 0.5 * df
        step = [lgamma_half_step(a)] if a >= 32.0 else [math.lgamma(a + 0.5), -math.lgamma(a)]
        return [-math.log(scale), -0.5 * math.log(df), -0.5 * math.log(math.pi)] + step
    if kind == CAUCHY:
        return [-math.log(math.pi * scale)]
    if kind == GENNORM:
        return [-math.log(2.0 * scale), -math.lgamma(1.0 / df), math.log(df)]
    raise ValueError(kind)


def log_norm(kind, scale, df):
    return math.fsum(log_norm_terms(kind, scale, df))


def elementwise(kind, loc, scale, df, N, theta, g, u, scale_rel=0.0):
    """Segment of an element-wise family (kinds 1-5; ``df`` is beta for GENNORM): the gradient after the hook,
    g' = g - (1/N) d log p / d theta_j, its per-element bound, the normalised log-density with its |.|-sum, and
    D = sum_j d log p / d scale (for a linked segment's hyper-parameter).  ``scale_rel``: relative allowance on ``scale``
    when it is the fp64 value of a hyper segment (``hyper_value``), 0 for a constant of the table.

    Per family, with d = theta - loc, u the working precision, locT = fl(loc) (|loc - locT| <= u |loc|, 0 when loc is a
    number of T -- the bound does not use that), the kernel's d_T = fl(theta - locT):

    NORMAL     g' = fma(d_T, c_T, g), c = 1 / (scale^2 N):
               u (|g'| + |c| (|loc| + 2 |d|))   [fma; c_T; loc's rounding; d_T's rounding]          + 2 scale_rel |c d|
    LAPLACE    g' = fma(sign(d_T), c_T, g), c = 1 / (scale N):  u (|g'| + |c|)   [fma; c_T]           + scale_rel |c|
               (the sign is exact when loc is a number of T or |d| > 2^-23 |loc|: the inputs see to that)
    STUDENT_T  g' = fma(d_T, q, g), q = fl(num_T / fl(fma(d_T, d_T, den_T))), num = (df + 1) / N, den = df scale^2;
    CAUCHY     = Student-t with df = 1.  Five roundings on the term t = d q (num_T, den_T, the inner fma, the division,
               d_T -- |dt/dd| <= q) and loc's rounding through d: u (|g'| + 5 |t| + q |loc|), plus |d| times the smallest
               subnormal of T where q underflows gradually (|d| = 3e30: q ~ 1e-62 is flushed to 0, the error IS t, which is
               below that)                                                                            + 2 scale_rel |t|
    GENNORM    g' = fma(sign(d_T) (T)pow(z_T, e_T), c_T, g), z_T = fl(|d_T| fl(1/scale)), e = beta - 1, c = beta / (scale N):
               z_T carries 3 roundings -> 3 |e| u on the power; pow itself, its conversion to T and c_T: 3 more:
               (3 |e| + 3) u |t|; and, where they apply, e's own rounding to T, |e_T - e| |log z| |t| (0 for beta = 0.5, 1,
               2, 8; beta = 1.7: 2.4e-8 |log z|), loc's rounding through z, |e| |locT - loc| / |d| |t| (the exact
               difference: 0 for a loc of T), the smallest subnormal times |c| (z^7 at z ~ 1e-6), and z_T's own gradual
               underflow, half the smallest subnormal absolute: |e| (subnormal / 2) / z |t|
                                                                                                      + |beta| scale_rel |t|
               The power is converted to T before the fma scales it: it is +-inf from T's largest number on.
    """
    th, g = np.asarray(theta, dtype=np.float64).reshape(-1), np.asarray(g, dtype=np.float64).reshape(-1)
    tiny = SUBNORMAL[u]
    with np.errstate(**_quiet):
        d = th - loc
        ad, z = np.abs(d), (th - loc) / scale
        if kind == NORMAL:
            c = 1.0 / (scale * scale * N)
            t = d * c
            new = g + t
            budget = u * (np.abs(new) + abs(c) * (abs(loc) + 2 * ad)) + 2 * scale_rel * np.abs(t)
            ref_own = U64 * (np.abs(new) + 5 * np.abs(t))             # d, scale^2, *N, 1/., d c; the sum
            lp_el = -0.5 * z * z
            dls, dls_abs = (z * z - 1.0) / scale, (z * z + 1.0) / scale
        elif kind == LAPLACE:
            c = 1.0 / (scale * N)
            t = np.sign(d) * c
            new = g + t
            budget = u * (np.abs(new) + abs(c)) + scale_rel * abs(c)
            ref_own = U64 * (np.abs(new) + 3 * abs(c))
            lp_el = -np.abs(z)
            dls, dls_abs = (np.abs(z) - 1.0) / scale, (np.abs(z) + 1.0) / scale
        elif kind in (STUDENT_T, CAUCHY):
            nu = 1.0 if kind == CAUCHY else df
            q = ((nu + 1.0) / N) / (d * d + nu * scale * scale)
            t = d * q
            new = g + t
            budget = u * (np.abs(new) + 5 * np.abs(t) + q * abs(loc)) + ad * tiny + 2 * scale_rel * np.abs(t)
            ref_own = U64 * (np.abs(new) + 7 * np.abs(t))
            zz = z * z
            lp_el = -0.5 * (nu + 1.0) * np.log1p(zz / nu)
            ratio = np.where(np.isinf(zz), nu + 1.0, (nu + 1.0) * zz / (nu + zz))
            dls, dls_abs = (ratio - 1.0) / scale, (ratio + 1.0) / scale
        elif kind == GENNORM:
            e, c = df - 1.0, df / (scale * N)
            az = ad / scale
            t = np.sign(d) * c * az ** e                  # 0 * inf = NaN at d == 0 for beta < 1, as the closed form
            new = g + t
            at = np.abs(t)
            log_z = np.abs(np.log(np.where(az > 0, az, 1.0)))
            budget = (u * (np.abs(new) + (3 * abs(e) + 3) * at) + abs(fround(e, u) - e) * log_z * at
                      + np.where(ad > 0, abs(e) * abs(fround(loc, u) - loc) / np.where(ad > 0, ad, 1.0), 0.0) * at
                      + tiny * abs(c) + abs(df) * scale_rel * at
                      + np.where(az > 0, abs(e) * 0.5 * tiny / np.where(az > 0, az, 1.0), 0.0) * at)
            # the power is converted to T BEFORE it is scaled by c: beyond T's largest number it is that infinity
            # whatever c makes of the exact product; and a z_T that has underflowed to 0 (theta one subnormal away from
            # loc = 0, divided by a scale > 2) makes a negative power infinite
            forced = (np.abs(az ** e) > LARGEST[u]) | ((e < 0) & (ad > 0) & (az < 0.5 * tiny))
            ref_own = U64 * (np.abs(new) + (6 + 2 * abs(e)) * at)
            lp_el = -az ** df
            dls = dls_abs = np.zeros_like(d)              # (the hook links no scale to a generalised normal)
        else:
            raise ValueError(f"not an element-wise weight kind: {kind}")
    if kind != GENNORM:
        forced = np.zeros(th.size, dtype=bool)
    ln = log_norm(kind, scale, df)
    n = th.size
    finite = np.isfinite(lp_el).all()
    unnorm = math.fsum(lp_el) if finite else float(np.sum(lp_el))
    D = math.fsum(dls) if np.isfinite(dls).all() else float(np.sum(dls))
    with np.errstate(**_quiet):
        el_abs = float(np.sum(np.abs(lp_el)))
        logp_abs = el_abs + n * abs(ln)
        dls_abs_sum = float(np.sum(dls_abs))
        # this file's own rounding of log p: every element's term is formed in <= 6 roundings (d, z, the square / power /
        # log1p, the scaling) and math.fsum adds them without error; every term of the normaliser is one or two library
        # calls and one or two roundings, 4 * 2^-53 of ITS magnitude (a normaliser of 0.28 made of terms of 2 carries
        # the rounding of the 2s), and is multiplied by numel
        logp_own = U64 * (6 * el_abs + 4 * n * sum(abs(t) for t in log_norm_terms(kind, scale, df)))
    return dict(g=new, bound=SAFETY * budget + ref_own, term=t, logp=unnorm + n * ln, logp_unnormalised=unnorm,
                logp_abs=logp_abs, logp_own=logp_own, log_norm=ln, numel=n, dls=D, dls_abs=dls_abs_sum, forced_inf=forced,
                # a linked segment's log-density moves with the scale's allowance: |d log p / d ln scale| <= scale sum|dls|
                logp_scale=scale_rel * scale * dls_abs_sum)


def logp_bound(ref):
    """|log p_kernel - log p_ref| for a constant-scale segment: numel * 2^-50 relative to the reference (fp64 evaluation
    of the stored values, accumulated in fp64 in any order), plus the reference's own rounding"""
    return ref["numel"] * LOGP_REL_PER_ELEMENT * abs(ref["logp"]) + ref["logp_own"]


def linked_logp_bound(ref):
    """the same for a segment whose scale is a hyper segment's value: the terms no longer share a sign with the
    normaliser -log(x) (x < 1 makes it positive), so the budget is on the |.|-sum, plus the scale's own allowance"""
    return ref["numel"] * LOGP_REL_PER_ELEMENT * ref["logp_abs"] + ref["logp_scale"] + ref["logp_own"]


def expected_overflow(ref, u):
    "elements whose exact result is beyond the working precision's largest number: the kernel gives that infinity"
    with np.errstate(**_quiet):
        return (np.abs(ref["g"]) > LARGEST[u]) | ref["forced_inf"]


def check_gradient(got, ref, u, what=""):
    """assert every element of ``got`` (the kernel's g, widened) within the family's bound; the NaN pattern and the
    infinities must be the reference's.  Returns the worst error / bound over the finite elements and its index."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    want, bound = ref["g"], ref["bound"]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern differs at {np.flatnonzero(np.isnan(got) != nan)[:8]}"
    over = expected_overflow(ref, u) & ~nan
    with np.errstate(**_quiet):
        assert np.array_equal(got[over], np.sign(want[over]) * np.inf), f"{what}: overflowing elements {np.flatnonzero(over)[:8]}"
    ok = ~nan & ~over
    with np.errstate(**_quiet):
        err = np.abs(got[ok] - want[ok])
        ratio = np.where(err == 0, 0.0, err / bound[ok])
    if ratio.size == 0:
        return 0.0, -1
    worst = int(np.argmax(ratio))
    idx = int(np.flatnonzero(ok)[worst])
    assert ratio[worst] <= 1.0, (f"{what}: element {idx}: got {got[idx]!r}, want {want[idx]!r}, |error| {err[worst]:.3e} = "
                                 f"{ratio[worst]:.3f} x bound {bound[idx]:.3e}; {int((ratio > 1).sum())} of {ratio.size} outside")
    return float(ratio[worst]), idx


def check_logp(got, want, bound, what=""):
    "non-finite exactly when the reference is (and then the same value); else within the bound.  Returns error / bound."
    if not math.isfinite(want):
        assert (math.isnan(got) and math.isnan(want)) or got == want, f"{what}: got {got!r}, want {want!r}"
        return 0.0
    assert math.isfinite(got), f"{what}: got {got!r}, want {want!r}"
    err = abs(got - want)
    assert err <= bound, f"{what}: got {got!r}, want {want!r}, |error| {err:.3e} > bound {bound:.3e}"
    return err / bound if bound > 0 else 0.0


# --------------------------------------------------------------------------------------------------- whitened kinds
def whitened(table, theta):
    """(log p, d log p / d theta, per-event sums or None) of a FILTER_WHITENED or MULTIVARIATE_T table (the dict of
    ``Prior.fused_filter_spec()`` / ``fused_mvt_spec()``; a table with an event geometry is the multivariate-t one) as
    include/sgmcmc_hip.h states the two kinds, in float64: z = (theta_f - mu) W per filter of P consecutive elements, then

    FILTER_WHITENED  log p = sum base(z) + lognorm per filter, gradient psi(z) W^T; all four bases, psi = 0 at z == 0 and
                     the double-Gamma log term as torch's xlogy
    MULTIVARIATE_T   M_e = sum of |z|^2 over event e's filters, element j in event (j / ev_div) % ev_mod,
                     log p = sum_e lognorm - (df + D) / 2 log1p(M_e / (df - 2)), gradient -(df + D) / (df - 2 + M_e) z W^T

    The gradient has theta's shape."""
    n = table["P"]
    th = np.asarray(theta, dtype=np.float64).reshape(-1, n)
    W = np.asarray(table["W"], dtype=np.float64)
    Z = (th - table["mu"]) @ W
    if "ev_div" in table:
        ev = (np.arange(th.size) // table["ev_div"]) % table["ev_mod"]
        M = np.bincount(ev[::n], weights=(Z * Z).sum(1), minlength=table["ev_mod"])
        lam, c = table["df"] - 2.0, table["df"] + table["ev_size"]
        lp = float(np.sum(table["lognorm"] - 0.5 * c * np.log1p(M / lam)))
        g = (-c / (lam + M[ev])) * (Z @ W.T).reshape(-1)
        return lp, g.reshape(np.shape(theta)), M
    a, s, beta, kind = np.abs(Z), table.get("base_scale", 1.0), table.get("beta", 2.0), table.get("base", BASE_NORMAL)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == BASE_NORMAL:
            base, psi = -0.5 * Z * Z, -Z
        elif kind == BASE_GENNORM:
            base, psi = -(a / s) ** beta, -np.sign(Z) * beta / s * (a / s) ** (beta - 1.0)
        elif kind == BASE_LAPLACE:
            base, psi = -a / s, -np.sign(Z) / s
        elif kind == BASE_DOUBLE_GAMMA:
            base = (0.0 if beta == 1.0 else (beta - 1.0) * np.log(a)) - a / s
            psi = (beta - 1.0) / Z - np.sign(Z) / s
        else:
            raise ValueError(kind)
    psi = np.where(Z == 0.0, 0.0, psi)
    return base.sum() + th.shape[0] * table["lognorm"], (psi @ W.T).reshape(np.shape(theta)), None


# --------------------------------------------------------------------------------------------------- kernel emulation
def emulate_fp32(kind, loc, scale, df, N, theta, g, coefficient_error=0.0):
    """numpy restatement of PriorCoef<float>::apply for NORMAL and STUDENT_T / CAUCHY (csrc/sgmcmc_hip.hip): what the
    mutation test perturbs.  An fma is the float64 product and sum rounded once to float32 (the product of two floats is
    exact in float64; the double rounding of the sum is beyond what the budget resolves)."""
    f32, f64 = np.float32, np.float64
    th, g = np.asarray(theta, dtype=f32), np.asarray(g, dtype=f32)
    with np.errstate(**_quiet):
        d = th - f32(loc)
        if kind == NORMAL:
            c = f32(1.0 / (scale * scale * N) * (1.0 + coefficient_error))
            return (d.astype(f64) * f64(c) + g.astype(f64)).astype(f32)
        nu = 1.0 if kind == CAUCHY else df
        num, den = f32((nu + 1.0) / N * (1.0 + coefficient_error)), f32(nu * scale * scale)
        inner = (d.astype(f64) * d.astype(f64) + f64(den)).astype(f32)
        q = (f64(num) / inner.astype(f64)).astype(f32)
        return (d.astype(f64) * q.astype(f64) + g.astype(f64)).astype(f32)
