"""numpy evaluator of the packed B-spline tables of prisim_amd/gains.py:pack_splines (the layout prisim_gains_eval_spline reads):
FITPACK's span search and fpbspl recursion in plain numpy, one point at a time."""
import numpy as NP


def fpbspl(t, k, x, l):
    h = NP.zeros(k + 1)
    h[0] = 1.0
    for j in range(1, k + 1):
        hh = h[:j].copy()
        h[0] = 0.0
        for i in range(1, j + 1):
            li, lj = l + i, l + i - j
            if t[li] == t[lj]:
                h[i] = 0.0
                continue
            f = hh[i - 1] / (t[li] - t[lj])
            h[i - 1] = h[i - 1] + f * (t[li] - x)
            h[i] = f * (x - t[lj])
    return h


def basis(t, k, x):
    n = t.size
    arg = min(max(x, t[k]), t[n - k - 1])
    l = k
    while not (arg < t[l + 1] or l == n - k - 2):
        l += 1
    return l - k, fpbspl(t, k, arg, l)


def eval_packed(packed, times, freqs):
    """(nt, nrows, nchan) complex values of every packed row at every (time, channel)."""
    kx, ky = packed['kx'], packed['ky']
    nrows = packed['nx'].size // 2
    out = NP.zeros((len(times), nrows, len(freqs)), dtype=NP.complex128)
    for r in range(nrows):
        vals = []
        for part in range(2):
            s = 2 * r + part
            tx = packed['knots'][packed['kx_off'][s]:packed['kx_off'][s] + packed['nx'][s]]
            ty = packed['knots'][packed['ky_off'][s]:packed['ky_off'][s] + packed['ny'][s]]
            ncy = ty.size - ky - 1
            c = packed['coefs'][packed['c_off'][s]:]
            v = NP.zeros((len(times), len(freqs)))
            for it, x in enumerate(times):
                lx, hx = basis(tx, kx, x)
                for jf, y in enumerate(freqs):
                    ly, hy = basis(ty, ky, y)
                    sp = 0.0
                    for i1 in range(kx + 1):
                        for j1 in range(ky + 1):
                            sp = sp + c[(lx + i1) * ncy + ly + j1] * hx[i1] * hy[j1]
                    v[it, jf] = sp
            vals.append(v)
        out[:, r, :] = vals[0] + 1j * vals[1]
    return out


GOLDEN = __import__('os').path.join(__import__('os').path.dirname(__import__('os').path.abspath(__file__)), 'golden', 'golden_gains.npz')
_KEYS = {'antenna': 'antenna-based', 'baseline': 'baseline-based'}


def load_golden():
    import json
    z = NP.load(GOLDEN)
    meta = json.loads(str(z['meta']))
    return z, {rec['name']: rec for rec in meta['cases']}


def bl_struct(pairs):
    n = max(len(str(a)) for p in pairs for a in p)
    return NP.asarray([tuple(str(a) for a in p) for p in pairs], dtype=[('A2', 'U%d' % n), ('A1', 'U%d' % n)])


def write_case(z, rec, path):
    """The gains file of one golden case, axes in the case's file ordering."""
    from prisim_amd import hdf5io
    axes = ['label', 'frequency', 'time']
    with hdf5io.File(path, 'w') as fo:
        for short, key in _KEYS.items():
            if ('%s/%s/gains' % (rec['name'], short)) not in z.files:
                continue
            order = rec['orderings'][key]
            g = z['%s/%s/gains' % (rec['name'], short)]
            fo.write(key + '/gains', NP.ascontiguousarray(NP.transpose(g, [axes.index(a) for a in order])))
            fo.write(key + '/ordering', NP.asarray(order))
            lab = z['%s/%s/label' % (rec['name'], short)]
            fo.write(key + '/label', bl_struct(lab.tolist()) if key == 'baseline-based' else lab)
            fo.write(key + '/frequency', z['%s/%s/frequency' % (rec['name'], short)])
            fo.write(key + '/time', z['%s/%s/time' % (rec['name'], short)])
