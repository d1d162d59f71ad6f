"""INTEGRATION.md is program text that a Symmer maintainer copies: its ctypes stub passes ints and c_doubles positionally, without
argtypes, so one argument out of order makes the document wrong without anything noticing.  Here the stub is PARSED (not run: importing
it calls symgpu_init(0), which needs a GPU) and every `_lib.symgpu_*(...)` call is held against include/symgpu.h and against
symmer_amd._lib.SIGNATURES — the table test_library_exports_every_declared_symbol ties to the header's names; this file also ties its
argument counts and type classes to the header's prototypes.  tests/test_gpu_c_abi.py runs the same stub on the device."""
import ast
import re

import pytest

from symmer_amd import _lib
from _integration_doc import doc_text, stub_source, header_text, header_prototypes, param_class

CLASS_OF = {_lib.P: 'ptr', _lib.PP: 'ptr', _lib.c_i64: 'i64', _lib.c_u64: 'u64', _lib.c_int: 'int', _lib.c_dbl: 'dbl'}
WRAPPERS = {'P': 'ptr', 'I64': 'i64', 'ctypes.byref': 'ptr', 'ctypes.c_double': 'dbl', 'ctypes.c_void_p': 'ptr', 'ctypes.c_int64': 'i64',
            'ctypes.c_uint64': 'u64'}


def _callee(node):
    """'P', 'I64', 'ctypes.byref', '_lib.symgpu_init', ... of a Call node, else None."""
    if not isinstance(node, ast.Call):
        return None
    f = node.func
    if isinstance(f, ast.Name):
        return f.id
    if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name):
        return f'{f.value.id}.{f.attr}'
    return None


def _lib_calls(source):
    tree = ast.parse(source)
    return [(c.split('.', 1)[1], node) for node in ast.walk(tree) for c in [_callee(node)] if c and c.startswith('_lib.symgpu_')]


def _arg_class(node):
    """The type class the literal shape of an argument shows: a wrapper call names it, anything else is a bare int expression."""
    return WRAPPERS.get(_callee(node), 'int')


def test_signature_table_matches_the_header_prototypes():
    protos = header_prototypes()
    assert len(protos) > 80 and 'symgpu_mul_cleanup' in protos and 'symgpu_last_error' in protos
    assert len(protos['symgpu_mul_cleanup']) == 14 and len(protos['symgpu_shutdown']) == 0
    for name, argtypes in _lib.SIGNATURES.items():
        assert name in protos, f'{name} is in SIGNATURES but not declared in include/symgpu.h'
        decls = protos[name]
        assert len(argtypes) == len(decls), f'{name}: SIGNATURES has {len(argtypes)} arguments, the header {len(decls)}: {decls}'
        for k, (t, d) in enumerate(zip(argtypes, decls)):
            assert CLASS_OF[t] == param_class(d), f'{name} argument {k}: SIGNATURES says {CLASS_OF[t]}, the header `{d}`'
    assert set(protos) - set(_lib.SIGNATURES) == {'symgpu_last_error'}


def test_stub_parses_and_calls_the_entry_points_it_claims():
    src = stub_source()
    assert "ctypes.CDLL('libsymgpu.so')" in src
    names = [n for n, _ in _lib_calls(src)]
    assert set(names) == {'symgpu_last_error', 'symgpu_init', 'symgpu_commutes', 'symgpu_cleanup', 'symgpu_mul_cleanup'}, names
    defs = {n.name for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef)}
    assert {'pack', 'unpack', 'commutes', 'cleanup', 'mul_cleanup', '_chk'} <= defs


@pytest.mark.parametrize('block', [0, 1])
def test_every_library_call_of_the_document_matches_the_prototype(block):
    """Block 0 is the stub of §1, block 1 the class sketch of §1b: argument count and, where the literal shape shows it, type class."""
    blocks = re.findall(r'```python\n(.*?)\n```', doc_text(), re.S)
    assert len(blocks) >= 2 and blocks[0] + '\n' == stub_source()
    protos = header_prototypes()
    calls = _lib_calls(blocks[block])
    assert calls
    for name, node in calls:
        assert name in protos, f'{name} is not declared in include/symgpu.h'
        assert not node.keywords, f'{name}: keyword arguments cannot cross a C boundary'
        table = [CLASS_OF[t] for t in _lib.SIGNATURES.get(name, [])]
        assert name in _lib.SIGNATURES or name == 'symgpu_last_error'
        assert len(node.args) == len(table) == len(protos[name]), \
            f'{name}: the document passes {len(node.args)} arguments, the prototype has {len(protos[name])}'
        for k, (arg, want) in enumerate(zip(node.args, table)):
            got = _arg_class(arg)
            if block == 1 and got == 'int' and want == 'ptr':
                # the sketch passes handles it keeps as ctypes.c_void_p objects (self._dev, out): a pointer-sized object, not an int literal
                assert isinstance(arg, (ast.Name, ast.Attribute, ast.Call)), (name, k, ast.dump(arg))
                continue
            assert got == want, f'{name} argument {k} (`{ast.unparse(arg)}`): the document passes {got}, the prototype wants {want} ({protos[name][k]})'


def test_every_name_the_document_mentions_is_declared():
    protos = header_prototypes()
    text = doc_text()
    seen = 0
    for m in re.finditer(r'(?<![A-Za-z0-9_])symgpu_\w+', text):
        name, rest = m.group(0), text[m.end():m.end() + 1]
        seen += 1
        if rest == '*' or name.endswith('_'):          # symgpu_comm_*, symgpu_commutes*, symgpu_init*: a family of names
            assert any(p.startswith(name) for p in protos), f'INTEGRATION.md names the family {name}*, the header declares none'
        else:
            assert name in protos, f'INTEGRATION.md names {name}, which include/symgpu.h does not declare'
    assert seen > 40
    defines = set(re.findall(r'#define\s+(SYMGPU_\w+)', header_text()))
    for name in set(re.findall(r'\bSYMGPU_E_\w+', text)):
        assert name in defines, f'INTEGRATION.md names {name}, which include/symgpu.h does not define'
