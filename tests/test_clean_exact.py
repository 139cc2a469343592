"""CPU: the exact-arithmetic row CLEAN (tests/clean_exact.py) and the input conditions of the delay CLEAN edge cases
(tests/clean_cases.py).  On the tie rows the numpy checker must equal the exact run bit for bit; the exact run in its rounding mode must
reproduce rows of the reference's fixtures; and the committed seeds must give rows whose deciding comparisons are either exact ties between
values equal up to signs or gaps no last bit can close, so that the device tests (tests/test_gpu_delay_clean_edges.py) excuse no row."""
import os

import numpy as NP
import pytest

import clean_cases as CC
import clean_checker as CK
import clean_exact as CE

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_clean.npz')


def _close(got, want, ulps):
    """NaN where NaN, else within ulps relative."""
    got, want = NP.asarray(got, dtype=float), NP.asarray(want, dtype=float)
    nan = NP.isnan(want)
    return NP.array_equal(NP.isnan(got), nan) and bool(NP.all(NP.abs(got[~nan] - want[~nan]) <= ulps * CK.ULP * NP.abs(want[~nan])))


@pytest.mark.parametrize('m,variant,repeats', CC.tie_batches())
def test_tie_rows_meet_the_input_conditions_and_the_checker_equals_the_exact_run(m, variant, repeats):
    b = CC.tie_batch(m, variant, repeats)
    cc, res, iters, flags, rms, gaps, sym = CC.tie_reference(m, variant, repeats)
    # conditions on the inputs (committed seeds): every tie is one any hypot resolves alike, every other decision is far from a last bit
    assert sym.all(), [b['ids'][r] for r in NP.flatnonzero(~sym)]
    assert (gaps > 1e-6).all(), [(b['ids'][r], gaps[r]) for r in NP.flatnonzero(~(gaps > 1e-6))]
    with NP.errstate(divide='ignore'):
        kcc, kres, kit, kfl, krms = CK.clean_rows(b['inp'], b['kern'], b['box'], b['gain'], b['maxiter'], b['threshold'], b['absolute'],
                                                  b['kidx'])
    assert NP.array_equal(kit, iters) and NP.array_equal(kfl, flags)
    assert NP.array_equal(kcc, cc) and NP.array_equal(kres, res)
    # |x - med| is the same exact difference on both sides; one hypot is within an ulp, the mean of two within one more rounding
    for r in range(len(b['ids'])):
        assert _close(krms[r], rms[r], 2), (b['ids'][r], krms[r], rms[r])


def test_the_tie_family_reaches_what_it_is_for():
    """Every stop condition, the rejected-threshold row, empty boxes (NaN inrms), <= 2 lags outside, equal inrms and outrms, and rows
    that run more than one iteration with ties."""
    flags, rms, iters = [], [], []
    for key in CC.tie_batches():
        out = CC.tie_reference(*key)
        flags.append(out[3]); rms.append(out[4]); iters.append(out[2])
    flags, rms, iters = NP.concatenate(flags), NP.concatenate(rms), NP.concatenate(iters)
    assert flags.size >= 300
    for bit in (1, 2, 4, 8, 16):
        assert NP.count_nonzero(flags & bit) >= 10, bit
    assert NP.count_nonzero(NP.isnan(rms[:, 0]) & (flags != 16)) >= 10
    assert NP.count_nonzero((rms[:, 0] == rms[:, 1]) & (rms[:, 0] > 0)) >= 5
    assert NP.count_nonzero(iters > 1) >= 100


def test_exact_run_details():
    # a zero gap between values that differ by more than signs is reported: |3 + 4j| = |4 + 3j| = |5|
    row = NP.array([3 + 4j, 4 + 3j, 1, 0, 0, 0, 0, 0], dtype=complex)
    kern = NP.zeros(8, dtype=complex)
    kern[0] = 1.0
    box = NP.array([1, 1, 1, 0, 0, 0, 0, 0])
    o = CE.clean_row(row, kern, box, 0.5, 1, 1.0 / 64)
    assert not o['ties_symmetric'] and o['iter'] == 1 and o['cc'][0] == 1.5 + 2j and o['exact']
    o = CE.clean_row(NP.array([3 + 4j, -3 + 4j, 1, 0, 0, 0, 0, 0]), kern, box, 0.5, 1, 1.0 / 64)
    assert o['ties_symmetric'] and o['cc'][0] == 1.5 + 2j and o['cc'][1] == 0
    # the peak halves to exactly the bound at the seventh iteration: cond1 holds with equality
    one = NP.zeros(8, dtype=complex)
    one[2] = 3 - 4j
    o = CE.clean_row(one, kern, NP.ones(8), 0.5, 100, 1.0 / 64)
    assert o['iter'] == 7 and o['cond1'] and not o['cond2'] and o['ties_symmetric']
    # gaps: 5 against sqrt(17), a near tie
    o = CE.clean_row(NP.array([5, 4 + 1j, 0, 0, 1, 2, 3, 4], dtype=complex), kern, box, 0.5, 1, 1.0 / 64)
    assert abs(o['min_gap'] - (1.0 - 17 ** 0.5 / 5)) < 1e-15
    # an irrational kernel peak has no exact run; the rounding mode takes it
    with pytest.raises(ValueError, match='irrational'):
        CE.clean_row(row, kern * (1 + 1j), box, 0.5, 1, 1.0 / 64)
    assert CE.clean_row(row, kern * (1 + 1j), box, 0.5, 1, 1.0 / 64, round_ops=True)['iter'] == 1
    # the checker's ValueError
    for thr, kind in ((1.0, 'relative'), (5.0, 'absolute'), (6.0, 'absolute')):
        with pytest.raises(ValueError, match='incompatible value'):
            CE.clean_row(row, kern, box, 0.5, 1, thr, kind)


@pytest.mark.parametrize('i', [4, 16, 18, 27, 28])
def test_exact_run_reproduces_reference_fixtures(i):
    """Rows of the reference's own fixtures with few iterations, in the rounding mode with the fused complex product of the numpy that
    made them: iter and conditions equal (the decisions of these rows are further than 4 ulp from a flip), rms within 4 ulp."""
    g = NP.load(GOLD)
    gain, maxiter, thr, absolute = g['params_%d' % i]
    o = CE.clean_row(g['inp_%d' % i], g['kernel_%d' % i], g['cbox_%d' % i], gain, int(maxiter), thr, 'absolute' if absolute else 'relative',
                     round_ops=True, fused=True)
    assert o['min_gap'] > 4 * CK.ULP and o['ties_symmetric']
    assert o['iter'] == int(g['iter_%d' % i])
    assert [o['cond1'], o['cond2'], o['cond3']] == list(g['cond_%d' % i])
    assert _close([o['inrms'], o['outrms']], g['rms_%d' % i], 4), (o['inrms'], o['outrms'], g['rms_%d' % i])
    scale = max(NP.abs(g['inp_%d' % i]).max(), 1e-300)
    assert NP.max(NP.abs(o['cc'] - g['cc_%d' % i])) <= 1e-13 * scale
    assert NP.max(NP.abs(o['res'] - g['res_%d' % i])) <= 1e-13 * scale


@pytest.mark.parametrize('m,nrows,per_row,maxiter', [(m, n, p, CC.SHIFTED_MAXITER) for m, n in CC.SHIFTED for p in (False, True)] +
                         [(m, 2, False, CC.LDS_EDGE_MAXITER) for m in CC.LDS_EDGE])
def test_shifted_kernel_rows_decide_far_from_a_last_bit(m, nrows, per_row, maxiter):
    """For the committed seed the checker's margin exceeds 64 ulp on every row, so the device comparison tolerates no row; and the
    kernels are what the family is for: peak off lag 0, complex."""
    b = CC.shifted_batch(m, nrows, per_row, maxiter)
    margins = CC.shifted_reference(m, nrows, per_row, maxiter)[5]
    assert (margins > 64 * CK.ULP).all(), margins.min()
    peak = NP.argmax(NP.abs(b['kern']), axis=1)
    assert (peak != 0).all()
    # the checker's divisor is the true modulus of the peak, rounded once: what the device divides by
    for k in b['kern']:
        assert NP.abs(k).max() == max(CE.rounded_modulus(v) for v in k[NP.abs(k) > 0.999 * NP.abs(k).max()])
    at = b['kern'][NP.arange(peak.size), peak]
    assert (NP.abs(at.real) > 0.1 * NP.abs(at)).all() and (NP.abs(at.imag) > 0.1 * NP.abs(at)).all()
    assert (len(set(peak.tolist())) > 1) == (per_row and nrows > 1)


@pytest.mark.parametrize('nchan,m', CC.DELAY_SHAPES)
def test_delay_chain_case_decides_far_from_a_last_bit(nchan, m):
    """The device forms the lag rows with another FFT, so they differ from the checker's by rounding: every decision of the checker
    must be far from that, and the five rows must not all do the same."""
    want = CC.delay_reference(nchan, m)
    assert want['margin'] > 1e-8, want['margin']
    c = CC.delay_case(nchan, m)
    assert len({bytes(b) for b in c['box']}) == (5 if m > 4 else 1) and len(set(c['kidx'].tolist())) == 3
    assert want['iters'].min() >= 1 and (m == 1 or len(set(want['iters'].ravel().tolist())) > 3)
