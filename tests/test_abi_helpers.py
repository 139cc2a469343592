"""The helpers the add-on wrappers of prisim_amd/_abi.py share: _stats_dict against the dict each wrapper used to write out by hand
(keys, Python types and values), the want bits, the route codes, the resample map, and the call by parameter name (_call_declared, Context._call) against a fake function.
No library is loaded."""
import numpy as NP
import pytest

from prisim_amd import _abi as A
from prisim_amd import dsp_readings

F, I, B, S = float, int, bool, str

# per stats struct: the call the wrapper makes, the dict it used to build by hand, and the keys with their types in order ('route' and
# 'phase_route' are typed by the case: a name where the table has the code, the code itself (route) or None (phase_route) where not)
CASES = {
    'clean': (A.PrisimCleanStats, lambda st: A._stats_dict(st, kernel_in_lds=bool),
              lambda st: {'device_ms': st.device_ms, 'clean_ms': st.clean_ms, 'sum_iter': int(st.sum_iter), 'rows': int(st.rows),
                          'waves_per_block': int(st.waves_per_block), 'kernel_in_lds': bool(st.kernel_in_lds),
                          'lds_bytes': int(st.lds_bytes)},
              [('device_ms', F), ('clean_ms', F), ('sum_iter', I), ('rows', I), ('waves_per_block', I), ('kernel_in_lds', B),
               ('lds_bytes', I)], None),
    'subband': (A.PrisimSubbandStats, lambda st: A._stats_dict(st, route=A.SUBBAND_ROUTES),
                lambda st: {'device_ms': st.device_ms, 'kernel_ms': st.kernel_ms, 'rows': int(st.rows),
                            'route': A.SUBBAND_ROUTES.get(st.route, st.route), 'lds_bytes': int(st.lds_bytes)},
                [('device_ms', F), ('kernel_ms', F), ('rows', I), ('route', None), ('lds_bytes', I)], A.SUBBAND_ROUTES),
    'runs': (A.PrisimRunsStats, lambda st: A._stats_dict(st, route=A.RUNS_ROUTES),
             lambda st: {'wall_ms': st.wall_ms, 'pairs': int(st.pairs), 'chunks': int(st.chunks), 'chunk_pairs': int(st.chunk_pairs),
                         'route': A.RUNS_ROUTES.get(st.route, st.route), 'streams': int(st.streams), 'tile': int(st.tile),
                         'lds_bytes': int(st.lds_bytes)},
             [('wall_ms', F), ('pairs', I), ('chunks', I), ('chunk_pairs', I), ('route', None), ('streams', I), ('tile', I),
              ('lds_bytes', I)], A.RUNS_ROUTES),
    'closure': (A.PrisimClosureStats, lambda st: dict(A._stats_dict(st, route=A.CLOSURE_ROUTES), resident=True),
                lambda st: {'wall_ms': st.wall_ms, 'kernel_ms': st.kernel_ms, 'triads': int(st.triads), 'chunks': int(st.chunks),
                            'chunk_triads': int(st.chunk_triads), 'kernel_bytes': int(st.kernel_bytes),
                            'download_bytes': int(st.download_bytes), 'route': A.CLOSURE_ROUTES.get(st.route, st.route),
                            'streams': int(st.streams), 'tile': int(st.tile), 'lds_bytes': int(st.lds_bytes), 'resident': True},
                [('wall_ms', F), ('kernel_ms', F), ('triads', I), ('chunks', I), ('chunk_triads', I), ('kernel_bytes', I),
                 ('download_bytes', I), ('route', None), ('streams', I), ('tile', I), ('lds_bytes', I), ('resident', B)],
                A.CLOSURE_ROUTES),
    'cpdelay': (A.PrisimCpdelayStats, lambda st: A._stats_dict(st, route=A.CPDELAY_ROUTES, phase_route=A.CLOSURE_ROUTES.get),
                lambda st: {'wall_ms': st.wall_ms, 'kernel_ms': st.kernel_ms, 'rows': int(st.rows), 'chunks': int(st.chunks),
                            'chunk_rows': int(st.chunk_rows), 'upload_bytes': int(st.upload_bytes),
                            'download_bytes': int(st.download_bytes), 'route': A.CPDELAY_ROUTES.get(st.route, st.route),
                            'phase_route': A.CLOSURE_ROUTES.get(st.phase_route), 'streams': int(st.streams), 'tile': int(st.tile),
                            'lds_bytes': int(st.lds_bytes)},
                [('wall_ms', F), ('kernel_ms', F), ('rows', I), ('chunks', I), ('chunk_rows', I), ('upload_bytes', I),
                 ('download_bytes', I), ('route', None), ('phase_route', None), ('streams', I), ('tile', I), ('lds_bytes', I)],
                A.CPDELAY_ROUTES),
    'cpbins': (A.PrisimCpbinsStats, lambda st: A._stats_dict(st, rename={'resident_in': 'resident'}, resident_in=bool),
               lambda st: {'wall_ms': st.wall_ms, 'kernel_ms': st.kernel_ms, 'elements': int(st.elements), 'chunks': int(st.chunks),
                           'chunk_triads': int(st.chunk_triads), 'kernel_bytes': int(st.kernel_bytes),
                           'upload_bytes': int(st.upload_bytes), 'download_bytes': int(st.download_bytes), 'max_bin': int(st.max_bin),
                           'resident': bool(st.resident_in)},
               [('wall_ms', F), ('kernel_ms', F), ('elements', I), ('chunks', I), ('chunk_triads', I), ('kernel_bytes', I),
                ('upload_bytes', I), ('download_bytes', I), ('max_bin', I), ('resident', B)], None),
    'cpdiff': (A.PrisimCpdiffStats, lambda st: A._stats_dict(st, rename={'resident_in': 'resident'}, resident_in=bool),
               lambda st: {'wall_ms': st.wall_ms, 'kernel_ms': st.kernel_ms, 'elements': int(st.elements), 'chunks': int(st.chunks),
                           'chunk_triads': int(st.chunk_triads), 'kernel_bytes': int(st.kernel_bytes),
                           'upload_bytes': int(st.upload_bytes), 'download_bytes': int(st.download_bytes),
                           'resident': bool(st.resident_in), 'ncomb': int(st.ncomb)},
               [('wall_ms', F), ('kernel_ms', F), ('elements', I), ('chunks', I), ('chunk_triads', I), ('kernel_bytes', I),
                ('upload_bytes', I), ('download_bytes', I), ('resident', B), ('ncomb', I)], None),
    'cpft': (A.PrisimCpftStats, lambda st: A._stats_dict(st, route=A.CPFT_ROUTES),
             lambda st: {'wall_ms': st.wall_ms, 'kernel_ms': st.kernel_ms, 'rows': int(st.rows), 'chunks': int(st.chunks),
                         'chunk_rows': int(st.chunk_rows), 'row_bytes': int(st.row_bytes), 'kernel_bytes': int(st.kernel_bytes),
                         'upload_bytes': int(st.upload_bytes), 'download_bytes': int(st.download_bytes),
                         'route': A.CPFT_ROUTES.get(st.route, st.route), 'streams': int(st.streams), 'group_rows': int(st.group_rows),
                         'lds_bytes': int(st.lds_bytes)},
             [('wall_ms', F), ('kernel_ms', F), ('rows', I), ('chunks', I), ('chunk_rows', I), ('row_bytes', I), ('kernel_bytes', I),
              ('upload_bytes', I), ('download_bytes', I), ('route', None), ('streams', I), ('group_rows', I), ('lds_bytes', I)],
             A.CPFT_ROUTES),
    'gains': (A.PrisimGainsStats, lambda st: A._stats_dict(st),
              lambda st: {'device_ms': st.device_ms, 'kernel_ms': st.kernel_ms, 'elements': int(st.elements)},
              [('device_ms', F), ('kernel_ms', F), ('elements', I)], None),
}


def filled(struct, **over):
    """The struct with distinct non-zero values: k + 1.5 in the k-th double, k + 2 in the k-th integer."""
    st = struct()
    for k, (name, ctype) in enumerate(struct._fields_):
        setattr(st, name, k + 1.5 if ctype is A.C.c_double else k + 2)
    for name, v in over.items():
        setattr(st, name, v)
    return st


def route_cases():
    for name, (struct, _, _, _, routes) in CASES.items():
        if routes is None:
            yield name, {}
            continue
        for code in list(routes) + [99]:                  # every named route, and a code the table lacks
            if name == 'cpdelay':
                for pcode in list(A.CLOSURE_ROUTES) + [-1]:
                    yield name, {'route': code, 'phase_route': pcode}
            else:
                yield name, {'route': code}


@pytest.mark.parametrize('name,over', list(route_cases()), ids=lambda v: v if isinstance(v, str) else '-'.join(str(x) for x in v.values()))
def test_stats_dict_is_the_handwritten_dict(name, over):
    struct, call, literal, keys, routes = CASES[name]
    st = filled(struct, **over)
    got, want = call(st), literal(st)
    assert list(got) == [k for k, _ in keys], 'keys and their order'
    assert 'reserved_' not in got
    assert got == want
    for k, typ in keys:
        assert type(got[k]) is type(want[k]), k
        if typ is not None:
            assert type(got[k]) is typ, k
    if routes is not None:
        assert type(got['route']) is (S if over['route'] in routes else I)
    if 'phase_route' in over:
        assert got['phase_route'] is None if over['phase_route'] not in A.CLOSURE_ROUTES else type(got['phase_route']) is S
    values = [v for v in got.values() if type(v) in (I, F)]
    assert len(set(values)) == len(values) and all(values), 'the fill is distinct and non-zero, so a swapped field shows'


def test_every_stats_struct_is_covered():
    structs = {v for k, v in vars(A).items() if k.startswith('Prisim') and k.endswith('Stats') and k != 'PrisimCommStats'}
    assert structs == {c[0] for c in CASES.values()}


def test_want_bits_and_route_codes():
    assert A._want_bits((), A.CPBINS_WANT) == 0
    assert A._want_bits(('wts', 'mad', 'wts'), A.CPBINS_WANT) == 65
    with pytest.raises(KeyError):
        A._want_bits(('wts', 'nope'), A.CPBINS_WANT)
    for routes, auto in ((A.SUBBAND_ROUTES, A.PRISIM_SUBBAND_AUTO), (A.CLOSURE_ROUTES, A.PRISIM_CLOSURE_AUTO),
                         (A.CPDELAY_ROUTES, A.PRISIM_CPDELAY_AUTO), (A.CPFT_ROUTES, A.PRISIM_CPFT_AUTO)):
        assert A._route_code('auto', routes) == auto == -1
        for code, rname in routes.items():
            assert A._route_code(rname, routes) == code
        with pytest.raises(KeyError):
            A._route_code('nope', routes)
    with pytest.raises(KeyError):
        A._route_code('direct', A.CPFT_ROUTES)


class FakeFunction(object):
    """Stands for a function of the library: records the positional arguments it is called with and returns 0."""

    def __init__(self):
        self.args = None

    def __call__(self, *args):
        self.args = args
        return 0


POWER = A.FUNCTIONS['prisim_closure_power'][1]       # ctx, n0, nwin, inner, spectra, scale, want, budget_bytes, three outputs, stats


def power_keywords():
    x, sc, out = NP.arange(12.0), NP.ones(2), NP.empty(6)
    st = A.PrisimCpdelayStats()
    return dict(ctx=A.C.c_void_p(7), n0=NP.int64(3), nwin=2.0, inner=True, spectra=x, scale=sc, want=NP.int32(4), budget_bytes=0,
                out_individual=None, out_auto=out, out_cross=None, stats=st)


def test_call_declared_restores_the_declared_order_and_marshals_by_class():
    kw = power_keywords()
    fn = FakeFunction()
    shuffled = {k: kw[k] for k in sorted(kw, key=lambda k: k[::-1])}
    assert list(shuffled) != [p for p, _ in POWER]
    assert A._call_declared(fn, 'prisim_closure_power', POWER, shuffled) == 0
    ctx, n0, nwin, inner, spectra, scale, want, budget, ind, auto, cross, stats = fn.args
    assert ctx is kw['ctx']                                                   # a ctypes object that is no struct goes as it is
    assert [(type(v), v) for v in (n0, nwin, inner, want, budget)] == [(int, 3), (int, 2), (int, 1), (int, 4), (int, 0)]
    assert (spectra, scale, auto) == (kw['spectra'].ctypes.data, kw['scale'].ctypes.data, kw['out_auto'].ctypes.data)
    assert ind is None and cross is None                                      # None goes as NULL
    assert type(stats) is type(A.C.byref(kw['stats'])) and stats._obj is kw['stats']    # a struct goes by reference
    # a double goes through float(); the instance a scalar pointer points to goes by reference; a pointer array as it is
    params = (('df', A.C.c_double), ('out', A.C.POINTER(A.C.c_void_p)), ('inputs', A.C.c_void_p), ('id', A.C.c_char_p))
    h, ptrs = A.C.c_void_p(), (A.C.c_void_p * 2)()
    A._call_declared(fn, 'f', params, dict(df=3, out=h, inputs=ptrs, id=b'x'))
    assert type(fn.args[0]) is float and fn.args[0] == 3.0 and fn.args[1]._obj is h and fn.args[2] is ptrs and fn.args[3] == b'x'


def test_call_declared_refuses_before_calling():
    fn = FakeFunction()
    kw = power_keywords()
    del kw['scale']
    with pytest.raises(TypeError, match=r"missing \['scale'\]"):
        A._call_declared(fn, 'prisim_closure_power', POWER, kw)
    with pytest.raises(TypeError, match=r"unknown \['scales'\]"):
        A._call_declared(fn, 'prisim_closure_power', POWER, dict(power_keywords(), scales=None))
    with pytest.raises(TypeError, match=r"missing \['scale'\], unknown \['scales'\]"):
        A._call_declared(fn, 'prisim_closure_power', POWER, dict(kw, scales=None))         # as many names as declared, one of them wrong
    with pytest.raises(ValueError, match='spectra must be a C-contiguous array'):
        A._call_declared(fn, 'prisim_closure_power', POWER, dict(power_keywords(), spectra=NP.arange(24.0)[::2]))
    assert fn.args is None


def test_context_call_fills_in_the_context_and_checks_the_code():
    """Context._call on a context that was never created: the library is a namespace of fake functions."""
    import types
    ctx = object.__new__(A.Context)
    fn = FakeFunction()
    ctx._lib, ctx._h = types.SimpleNamespace(prisim_closure_power=fn, prisim_cphase_stack_free=lambda stack: None,
                                             prisim_hip_last_error=lambda h: b'refused'), A.C.c_void_p(5)
    kw = power_keywords()
    del kw['ctx']
    ctx._call('prisim_closure_power', **kw)
    assert fn.args[0] is ctx._h and len(fn.args) == len(POWER)
    ctx._call('prisim_cphase_stack_free', stack=A.C.c_void_p(9))              # void: nothing to check, and no context to pass
    ctx._lib.prisim_closure_power = lambda *args: A.PRISIM_EINVAL
    with pytest.raises(ValueError, match='prisim_closure_power failed: refused'):
        ctx._call('prisim_closure_power', **kw)
    with pytest.raises(KeyError):
        ctx._call('prisim_no_such_entry')
    ctx._h = None                                                             # (nothing for __del__ to destroy)


DELAY_PADS = ('0', '0.05', '0.1', '0.2', '0.25', '0.3', '0.33', '0.4', '0.5', '0.6', '0.7', '0.75', '0.8', '0.9', '1', '1.1', '1.25', '1.5',
              '2', '2.5', '3')


def test_delay_nout_is_the_exact_count_and_arange_is_not():
    """delay_nout (the library's rule, delay_geom in csrc/capi.cpp) against the exact count of j >= 0 with j (1 + pad) < nfft, the pad
    taken as the decimal written, for 2 <= nchan < 2100 and 21 pads.  numpy's len(arange(0, nfft, 1 + pad)), which sized the host
    arrays before, is one more at pad 0.4 (1400 / 1.4 evaluates to 1000.0000000000001) and nowhere less; its extra position is >= nfft,
    so no sample of the spectrum is lost by following the library."""
    from fractions import Fraction
    longer = []
    for ps in DELAY_PADS:
        pad, fpad = float(ps), Fraction(ps)
        for nchan in range(2, 2100):
            nfft = nchan + int(nchan * pad)
            q = Fraction(nfft) / (1 + fpad)
            exact = -((-q.numerator) // q.denominator)                     # ceil
            assert A.delay_nout(nchan, pad) == exact, (nchan, ps)
            pos = NP.arange(0, nfft, 1.0 + pad)
            if pos.size != exact:
                assert pos.size == exact + 1 and pos[-1] >= nfft, (nchan, ps, pos.size, exact)
                longer.append((nchan, ps))
    assert NP.arange(0, 1400, 1.4).size == 1001 and A.delay_nout(1000, 0.4) == 1000
    assert len(longer) == 102 and {ps for _, ps in longer} == {'0.4'}
    assert {15, 30, 60, 115, 120, 125, 225, 230, 235, 240, 245, 250, 255, 1000} <= {n for n, _ in longer}
    assert A.delay_nout(64, -1.0) == 64                                   # a negative pad is no pad, as in the library


def test_resample_map_helper():
    assert A._resample_map(False, 16, 8) == (0, None, None, None)
    assert A._resample_map(0, 16, 8) == (0, None, None, None)
    nmap, mo, mi, mw = A._resample_map(True, 16, 6)
    ref = dsp_readings.resample_map(16, 6)
    assert nmap == len(ref[0]) > 0
    for got, want in zip((mo, mi, mw), ref):
        assert got.flags['C_CONTIGUOUS'] and got.dtype == NP.asarray(want).dtype and NP.array_equal(got, want)
