"""Helpers for the tests that treat INTEGRATION.md and include/symgpu.h as the things under test: the ctypes stub of §1 as source text,
and the prototypes of the header as (name -> list of parameter declarations).  Text processing only; nothing here loads the library."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = os.path.join(ROOT, 'INTEGRATION.md')
HEADER = os.path.join(ROOT, 'include', 'symgpu.h')


def doc_text():
    with open(DOC) as f:
        return f.read()


def stub_source():
    """The first fenced ```python block of INTEGRATION.md §1."""
    text = doc_text()
    start = text.index('## 1. The stub')
    m = re.search(r'```python\n(.*?)\n```', text[start:], re.S)
    assert m, 'INTEGRATION.md §1 has no ```python block'
    return m.group(1) + '\n'


def header_text():
    with open(HEADER) as f:
        return f.read()


def header_prototypes():
    """name -> list of parameter declarations (comments stripped), for every `int symgpu_*(...)` / `const char *symgpu_*(...)` prototype."""
    text = re.sub(r'/\*.*?\*/', ' ', header_text(), flags=re.S)
    protos = {}
    for m in re.finditer(r'\b(?:int|const\s+char\s*\*)\s*(symgpu_\w+)\s*\(([^()]*)\)\s*;', text):
        params = ' '.join(m.group(2).split())
        protos[m.group(1)] = [] if params in ('', 'void') else [p.strip() for p in params.split(',')]
    return protos


def param_class(decl):
    """The type class of one parameter declaration of the header: 'ptr', 'i64', 'u64', 'int', 'dbl' or 'float'."""
    if '*' in decl or '[' in decl or re.match(r'(const\s+)?symgpu_(op|csr)_t\b', decl):
        return 'ptr'                                   # symgpu_op_t / symgpu_csr_t are pointers to opaque structs
    base = re.sub(r'\bconst\b', '', decl).split()
    return {'int64_t': 'i64', 'uint64_t': 'u64', 'int': 'int', 'double': 'dbl', 'float': 'float'}[base[0]]
