"""CPU: the whole ctypes binding (prisim_amd/_abi.py) held to the headers under include/, written once for every header found there --
the struct mirrors (STRUCTS) against a gcc-compiled program and the text of the struct bodies, the PRISIM_* constants in name and
value, the prototype table (FUNCTIONS) against the text of the declarations, what the built library exports, and that no C++
exception crosses the ABI.  A new header, struct, constant or function is covered with no new test."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

from prisim_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = sorted(glob.glob(os.path.join(ROOT, 'include', '*.h')))
SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64, 'double': C.c_double}
RETURNS = {'int': C.c_int, 'void': None, 'const char*': C.c_char_p}
CANNOT_THROW = ('prisim_hip_comm_last_error', 'prisim_gains_table_shape')      # int entries whose bodies are not run through guarded()


def _text(path):
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S))


def _declaration(decl):
    """(base type, pointer depth, name) of one parameter or field: const dropped, a [N] suffix counted as one pointer level."""
    m = re.match(r'^(?:const\s+)?(\w+)\s*((?:\*|\bconst\b|\s)*)(\w+)\s*(\[\w+\])?$', ' '.join(decl.split()))
    assert m, decl
    return m.group(1), m.group(2).count('*') + (1 if m.group(4) else 0), m.group(3)


def _parse(path):
    """What one header declares: structs {name: [field names]}, constants [names], functions [(name, return, [(base, depth, name)])]."""
    txt = _text(path)
    structs = {}
    for tag, body, name in re.findall(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;', txt, flags=re.S):
        assert tag == name, (tag, name)
        # `int64_t a, b;` declares two fields: the first with its type, the others bare
        structs[name] = [_declaration(part if i == 0 else 'int ' + part)[2]
                         for d in body.split(';') if d.strip() for i, part in enumerate(d.split(','))]
    constants = [n for n, rest in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(PRISIM_\w+)\b(?!\()([^\n]*)', txt, flags=re.M)
                 if not (n.endswith('_H') and not rest.strip())]                     # include guards aside
    for body in re.findall(r'\benum\b[^{;]*\{(.*?)\}', txt, flags=re.S):
        constants += [re.match(r'\s*(\w+)', item).group(1) for item in body.split(',') if item.strip()]
    functions = []
    for ret, name, params in re.findall(r'^(int|void|const char\*)\s+(prisim_\w+)\s*\(([^)]*)\)\s*;', txt, flags=re.M | re.S):
        params = ' '.join(params.split())
        functions.append((name, ret, [] if params == 'void' else [_declaration(p) for p in params.split(',')]))
    return structs, constants, functions


PARSED = {os.path.basename(h): _parse(h) for h in HEADERS}
HEADER_STRUCTS = {name: fields for structs, _, _ in PARSED.values() for name, fields in structs.items()}
HEADER_CONSTANTS = [n for _, constants, _ in PARSED.values() for n in constants]


@pytest.fixture(scope='module')
def compiled(tmp_path_factory):
    """What gcc makes of the headers: {'<struct>': [sizeof], '<struct>.<field>': [offsetof, sizeof], '<constant>': [value]}."""
    lines = ['#include <stdio.h>', '#include <stddef.h>'] + ['#include "%s"' % h for h in sorted(PARSED)] + ['int main(void) {']
    for cname, fields in sorted(HEADER_STRUCTS.items()):
        lines.append('  printf("{0} %zu\\n", sizeof({0}));'.format(cname))
        for f in fields:
            lines.append('  printf("{0}.{1} %zu %zu\\n", offsetof({0}, {1}), sizeof((({0}*)0)->{1}));'.format(cname, f))
    lines += ['  printf("{0} %lld\\n", (long long)({0}));'.format(n) for n in HEADER_CONSTANTS]
    lines += ['  return 0;', '}']
    tmp = tmp_path_factory.mktemp('abi_headers')
    src, exe = tmp / 'abi.c', tmp / 'abi'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in subprocess.check_output([str(exe)]).decode().splitlines()}


def test_the_headers_are_found_and_parsed():
    assert len(PARSED) >= 15 and sorted(PARSED) == sorted(_abi.HEADER_EXPORTS)
    assert sum(len(f) for _, _, f in PARSED.values()) >= 74 and len(HEADER_STRUCTS) >= 25 and len(HEADER_CONSTANTS) >= 108
    assert len(set(HEADER_CONSTANTS)) == len(HEADER_CONSTANTS)


def test_every_struct_has_its_mirror_field_by_field(compiled):
    assert sorted(HEADER_STRUCTS) == sorted(_abi.STRUCTS)
    assert len(set(_abi.STRUCTS.values())) == len(_abi.STRUCTS)
    for cname, cls in _abi.STRUCTS.items():
        # the names from the text: a field missing from the mirror fails even where padding hides it
        assert [f for f, _ in cls._fields_] == HEADER_STRUCTS[cname], cname
        assert compiled[cname] == [C.sizeof(cls)], cname
        for fname, ftype in cls._fields_:
            assert compiled[cname + '.' + fname] == [getattr(cls, fname).offset, C.sizeof(ftype)], (cname, fname)


def test_every_constant_has_its_mirror_in_name_and_value(compiled):
    mirrored = {k: v for k, v in vars(_abi).items() if k.startswith('PRISIM_') and isinstance(v, int)}
    assert sorted(mirrored) == sorted(HEADER_CONSTANTS)
    for name, value in mirrored.items():
        assert compiled[name] == [value], name


def _expected_class(base, depth, declared):
    """The ctypes class a parameter of this C type must be declared with; where the header leaves a choice (a pointer to scalars or
    to an opaque type: void* or a typed pointer), `declared` if it is one of them."""
    if depth == 0:
        return SCALARS[base]
    if depth == 1 and base == 'char':
        return C.c_char_p
    if depth == 1 and base in _abi.STRUCTS:
        return C.POINTER(_abi.STRUCTS[base])                     # a mirrored struct is never passed as a bare pointer
    typed = C.POINTER(SCALARS[base]) if depth == 1 and base in SCALARS else C.POINTER(C.c_void_p) if depth == 2 else None
    return declared if declared in (C.c_void_p, typed) else C.c_void_p


def test_every_prototype_agrees_with_its_header():
    declared = {name: (header, ret, params) for header, (_, _, functions) in PARSED.items() for name, ret, params in functions}
    assert sorted(declared) == sorted(_abi.FUNCTIONS)
    for header, (_, _, functions) in PARSED.items():
        assert _abi.HEADER_EXPORTS[header] == tuple(name for name, _, _ in functions), header     # the header's functions, in its order
    for name, (header, ret, params) in declared.items():
        restype, mirror = _abi.FUNCTIONS[name]
        assert restype is RETURNS[ret], name
        assert [p for p, _ in mirror] == [p for _, _, p in params], name                          # count, names and order
        for (pname, ctype), (base, depth, _) in zip(mirror, params):
            assert ctype is _expected_class(base, depth, ctype), (name, pname)


def test_export_tuples_are_the_groups_of_the_table():
    names = {'prisim_hip.h': 'EXPORTS'}
    for header in _abi.HEADER_EXPORTS:
        tup = getattr(_abi, names.get(header, header[len('prisim_'):-len('.h')].upper() + '_EXPORTS'))
        assert tup == _abi.HEADER_EXPORTS[header] and len(tup) >= 1, header
    assert sum(len(t) for t in _abi.HEADER_EXPORTS.values()) == len(_abi.FUNCTIONS)                # no function in two headers


def test_library_exports_and_declares_every_function():
    lib = _abi.load_library()
    for name, (restype, params) in _abi.FUNCTIONS.items():
        assert hasattr(lib, name), 'libprisim_hip.so does not export ' + name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == [c for _, c in params], name


def test_no_cpp_exception_crosses_the_abi():
    """Every `int prisim_*` entry of the library's sources runs its body through guarded() (bad_alloc -> PRISIM_ENOMEM, anything else ->
    PRISIM_EINTERNAL); the void / const char* entries cannot throw by construction, and neither can the two named here."""
    src = ''.join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, 'prisim_amd', 'csrc', '*.cpp')) +
                                                 glob.glob(os.path.join(ROOT, 'prisim_amd', 'csrc_*', '*.hip'))))
    entries = re.findall(r'^int (prisim_\w+)\(', src, flags=re.M)
    assert sorted(entries) == sorted(n for n, (restype, _) in _abi.FUNCTIONS.items() if restype is C.c_int)
    for name in entries:
        body = src[src.index('int %s(' % name):]
        if name in CANNOT_THROW:
            assert 'return guarded(' not in body[:body.index('\n}\n')], name
            continue
        assert 'return guarded(' in body[:body.index('{') + 200], name
    # prisim_hip_comm_last_error: a watchdog thread calls it while another thread is inside RCCL: one snprintf into the caller's buffer,
    # no allocation, no context, no HIP call -- nothing in it can throw, and it must not wait for anything
    body = src[src.index('int prisim_hip_comm_last_error('):]
    body = body[:body.index('\n}\n')]
    assert 'snprintf' in body and 'std::string' not in body and 'hip' not in body.replace('prisim_hip', '')
    # host allocations of caller-sized vectors run inside the guard: a failed one comes back as a code, e.g. from host_alloc
    lib = _abi.load_library()
    p = C.c_void_p()
    assert lib.prisim_hip_host_alloc(-5, C.byref(p)) == _abi.PRISIM_EINVAL and not p.value
