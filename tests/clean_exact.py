"""Row CLEAN in exact arithmetic (TEST INFRASTRUCTURE), with the contract of clean_checker.clean_row: the arbiter of rows with ties.

numpy's complex abs is not correctly rounded, so on a row whose deciding comparisons are between equal moduli "the checker says tie"
is no ground truth.  Here every value is a pair of fractions.Fraction, every comparison of moduli (the argmax over the box, |maxres|
against the threshold, the ordering of the absolute deviations) is made on squared moduli, exactly, the complex median is taken in
numpy's lexicographic order, and the two medians of absolute deviations are formed from decimal square roots at PREC digits, compared
at that precision and only then rounded to double.

Besides the checker's entries a run reports
  min_gap         the smallest non-zero relative gap of a deciding comparison (best against second-best modulus in the box, |maxres|
                  against the bound, inrms against outrms): what a last-bit difference of a device could flip;
  ties_symmetric  True when every zero-gap deciding comparison was between values equal up to the signs of their components, the only
                  ties every hypot resolves alike.  A zero gap against the bound counts only where the bound is the peak scaled by a
                  power of two (see scaled_copy); any other bound is a rounded product;
  exact           True when every cc and res is a double (no operation of the double pipeline rounded on this row).

round_ops=True rounds every product, sum and difference to double as the double pipeline does (the decisions stay exact): the mode
for rows of continuous data, where exact residuals would grow by a hundred bits per iteration.  fused=True rounds the complex product
ccval * kernel as fma(ar, br, -(ai bi)), fma(ar, bi, ai br), numpy's vector loop on processors with fused multiply-add; the default is
four products and two sums, each rounded."""
import decimal
import math
from fractions import Fraction

import numpy as NP

PREC = 100
_CTX = decimal.Context(prec=PREC)
_TIE = decimal.Decimal(10) ** (20 - PREC)            # relative gap below which two values at PREC digits are one number


def _dec(fr):
    return _CTX.divide(decimal.Decimal(fr.numerator), decimal.Decimal(fr.denominator))


def _root(fr):
    return _CTX.sqrt(_dec(fr))


def rounded_modulus(z):
    """|z| of a complex double, correctly rounded."""
    z = complex(z)
    with decimal.localcontext(_CTX):
        return float(_root(Fraction(z.real) ** 2 + Fraction(z.imag) ** 2))


def _exact_root(fr):
    """sqrt of a Fraction when it is rational, else None."""
    n, d = math.isqrt(fr.numerator), math.isqrt(fr.denominator)
    return Fraction(n, d) if n * n == fr.numerator and d * d == fr.denominator else None


def _same(fr):
    return fr


def _to_double(fr):
    return Fraction(float(fr))


def _pairs(z):
    z = NP.asarray(z, dtype=NP.complex128).ravel()
    return [(Fraction(float(v.real)), Fraction(float(v.imag))) for v in z]


def _d2(v):
    return v[0] * v[0] + v[1] * v[1]


def _mad(vals, rd):
    """median(|x - median(x)|) of a list of pairs: (value at PREC digits, {middle squared deviation: set of (|dx|, |dy|) attaining it});
    None for an empty list."""
    n = len(vals)
    if n == 0:
        return None
    s = sorted(vals)                                             # lexicographic: real, then imaginary; -0 == +0
    h = n // 2
    med = s[h] if n & 1 else (rd(s[h - 1][0] + s[h][0]) / 2, rd(s[h - 1][1] + s[h][1]) / 2)
    dev = [(abs(rd(v[0] - med[0])), abs(rd(v[1] - med[1]))) for v in vals]
    sq = sorted(_d2(d) for d in dev)
    mids = [sq[h]] if n & 1 else [sq[h - 1], sq[h]]
    value = _root(mids[0]) if n & 1 else (_root(mids[0]) + _root(mids[1])) / 2
    who = {q: {d for d in dev if _d2(d) == q} for q in mids}
    return value, who, tuple(mids)


def clean_row(inp, kernel, cbox, gain=0.1, maxiter=10000, threshold=5e-3, threshold_type='relative', round_ops=False, fused=False):
    with decimal.localcontext(_CTX):                             # Decimal operators take the thread's context, not _CTX
        return _clean_row(inp, kernel, cbox, gain, maxiter, threshold, threshold_type, round_ops, fused)


def _clean_row(inp, kernel, cbox, gain, maxiter, threshold, threshold_type, round_ops, fused):
    """One row.  Returns a dict: cc, res (complex128), iter, cond1, cond2, cond3, inrms, outrms (doubles; outrms None when <= 2 lags are
    outside the box, inrms NaN for an empty box), min_gap, ties_symmetric, exact.  Raises ValueError where the checker does."""
    rd = _to_double if round_ops else _same
    fu = _same if fused else rd                                  # the first product of each part, unrounded when fused
    g = Fraction(float(gain))
    x = _pairs(inp)
    k = _pairs(kernel)
    m = len(x)
    box = NP.asarray(cbox).ravel() > 0
    sym = True
    # kernel /= max|kernel| (:206): times the reciprocal of the peak modulus, as numpy divides a complex array by a float
    kpeak2 = max(_d2(v) for v in k)
    r = _exact_root(kpeak2)
    if r is None:
        if not round_ops:
            raise ValueError('the kernel peak has an irrational modulus: no exact run')
        r = Fraction(float(_root(kpeak2)))
    scl = rd(1 / r)
    k = [(rd(a * scl), rd(b * scl)) for a, b in k]
    kd2 = [_d2(v) for v in k]
    kmaxind = kd2.index(max(kd2))                                # :207, the first of equals
    if any(kd2[j] == kd2[kmaxind] and (abs(k[j][0]), abs(k[j][1])) != (abs(k[kmaxind][0]), abs(k[kmaxind][1])) for j in range(m)):
        sym = False
    taps = [(j, k[j]) for j in range(m) if kd2[j] != 0]
    inmax2 = max(_d2(v) for v in x)
    if threshold_type == 'relative':                             # :224-230
        if threshold >= 1.0:
            raise ValueError('incompatible value specified for threshold')
        bound2 = Fraction(float(threshold)) ** 2 * inmax2
    else:
        bound2 = Fraction(float(threshold)) ** 2
        if inmax2 == 0 or bound2 >= inmax2:
            raise ValueError('incompatible value specified for threshold')
    lolim = Fraction(float(threshold))
    pow2 = threshold_type == 'relative' and lolim.numerator == 1 and lolim.denominator & (lolim.denominator - 1) == 0
    peaks = {(abs(v[0]) * lolim, abs(v[1]) * lolim) for v in x if _d2(v) == inmax2}

    def scaled_copy(v):
        # a relative threshold that is a power of two scales the peak exactly: the bound and |v| are then one double when v is the
        # peak's components times the threshold, up to signs.  Any other zero gap against the bound meets a rounded product.
        return pow2 and (abs(v[0]), abs(v[1])) in peaks

    inside = [j for j in range(m) if box[j]]
    outside = [j for j in range(m) if not box[j]]
    nout = len(outside)
    cc = [(Fraction(0), Fraction(0))] * m
    res = list(x)
    itr = 0
    cond1 = cond2 = cond3 = False
    vin = vout = None
    min_gap = float('inf')
    while True:                                                  # :280-313
        itr += 1
        best = max((_d2(res[j]) for j in inside), default=Fraction(0))
        if best > 0:
            tied = [j for j in inside if _d2(res[j]) == best]
            ind = tied[0]
            if any((abs(res[j][0]), abs(res[j][1])) != (abs(res[ind][0]), abs(res[ind][1])) for j in tied[1:]):
                sym = False
            if len(inside) > len(tied):
                second = max(_d2(res[j]) for j in inside if _d2(res[j]) != best)
                min_gap = min(min_gap, 1.0 - math.sqrt(float(second / best)))
        else:
            ind = 0                                              # NP.argmax of all zeros
        maxres = res[ind]
        cv = (rd(g * maxres[0]), rd(g * maxres[1]))
        cc[ind] = (rd(cc[ind][0] + cv[0]), rd(cc[ind][1] + cv[1]))
        s = ind - kmaxind
        for j, (kx, ky) in taps:                                 # res - ccval * roll(kernel, indmaxres - kmaxind)
            p = (j + s) % m
            tr = rd(fu(cv[0] * kx) - rd(cv[1] * ky))
            ti = rd(fu(cv[0] * ky) + rd(cv[1] * kx))
            res[p] = (rd(res[p][0] - tr), rd(res[p][1] - ti))
        top2 = _d2(maxres)
        cond1 = top2 <= bound2                                   # :300
        if bound2 > 0:
            if top2 == bound2:
                sym = sym and scaled_copy(maxres)
            else:
                min_gap = min(min_gap, abs(math.sqrt(float(top2 / bound2)) - 1.0))
        cond2 = itr >= maxiter
        if nout > 2:
            vin = _mad([res[j] for j in inside], rd)
            vout = _mad([res[j] for j in outside], rd)           # :306
            if vin is None:
                cond3 = False                                    # NaN <= outrms
            else:
                a, b = vin[0], vout[0]
                big = max(a, b)
                if big == 0 or abs(a - b) <= _TIE * big:
                    cond3 = True
                    # the same middle deviations on both sides, each attained by one (|dx|, |dy|) only: the same doubles whatever hypot
                    if set(vin[2]) != set(vout[2]) or any(len(vin[1][q]) != 1 or vin[1][q] != vout[1][q] for q in vin[2]):
                        sym = False
                else:
                    cond3 = a < b                                # :307
                    if b > 0:
                        min_gap = min(min_gap, float(abs(a - b) / b))
        if cond1 or cond2 or cond3:
            break
    if nout <= 2:
        vin = _mad([res[j] for j in inside], rd)
    exact = all(Fraction(float(c)) == c for v in cc + res for c in v)
    out = {'cc': NP.array([complex(float(a), float(b)) for a, b in cc]), 'res': NP.array([complex(float(a), float(b)) for a, b in res]),
           'iter': itr, 'cond1': bool(cond1), 'cond2': bool(cond2), 'cond3': bool(cond3),
           'inrms': float('nan') if vin is None else float(vin[0]), 'outrms': None if nout <= 2 else float(vout[0]),
           'min_gap': min_gap, 'ties_symmetric': sym, 'exact': exact}
    return out



def clean_rows(inp, kern, cbox, gain, maxiter, threshold, absolute=False, kidx=None, round_ops=False):
    """clean_checker.clean_rows by the exact run: cc, res, iters, flags, rms, and the per-row min_gap and ties_symmetric (inf and True on
    a row the threshold rejects)."""
    inp = NP.asarray(inp, dtype=NP.complex128)
    kern = NP.asarray(kern, dtype=NP.complex128).reshape(-1, inp.shape[1])
    nrows = inp.shape[0]
    cc, res = NP.zeros_like(inp), NP.zeros_like(inp)
    iters, flags, rms = NP.zeros(nrows, NP.int32), NP.zeros(nrows, NP.int32), NP.full((nrows, 2), NP.nan)
    gaps, sym = NP.full(nrows, NP.inf), NP.ones(nrows, dtype=bool)
    for r in range(nrows):
        try:
            o = clean_row(inp[r], kern[0 if kidx is None else kidx[r]], cbox[r], gain, maxiter, threshold,
                          'absolute' if absolute else 'relative', round_ops)
        except ValueError:
            res[r], flags[r] = inp[r], 16
            continue
        cc[r], res[r], iters[r] = o['cc'], o['res'], o['iter']
        flags[r] = o['cond1'] * 1 | o['cond2'] * 2 | o['cond3'] * 4 | (o['outrms'] is None) * 8
        rms[r] = (o['inrms'], NP.nan if o['outrms'] is None else o['outrms'])
        gaps[r], sym[r] = o['min_gap'], o['ties_symmetric'] and o['exact']
    return cc, res, iters, flags, rms, gaps, sym
