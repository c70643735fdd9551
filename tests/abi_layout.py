"""What the C compiler makes of include/gq.h, for the tests that hold the ctypes binding (gym_quadruped_amd/cabi.py, _lib.py) to it: the
layout of every struct from ONE generated program, compiled once per session, and the header's constants and prototypes from its text."""
import ctypes
import functools
import re
import subprocess
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def mirrors(module):
    """every ctypes.Structure the module defines, in the order of definition"""
    return [t for t in vars(module).values() if isinstance(t, type) and issubclass(t, ctypes.Structure) and t.__module__ == module.__name__]


@functools.lru_cache(maxsize=None)
def c_layout(structs):
    """structs: a tuple of ctypes.Structure classes named as in gq.h -> {name: (sizeof, {field: offsetof})} as gcc sees them"""
    lines = [f'printf("{t.__name__} %zu\\n", sizeof({t.__name__}));' for t in structs]
    lines += [f'printf("{t.__name__}.{f} %zu\\n", offsetof({t.__name__}, {f}));' for t in structs for f, *_ in t._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gq.h"\nint main(void) {\n' + '\n'.join(lines) + '\nreturn 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / 'a.c').write_text(src)
        subprocess.run(['gcc', '-I', str(ROOT / 'include'), str(Path(d) / 'a.c'), '-o', str(Path(d) / 'a')], check=True)
        out = dict(ln.split() for ln in subprocess.run([str(Path(d) / 'a')], check=True, capture_output=True, text=True).stdout.splitlines())
    return {t.__name__: (int(out[t.__name__]), {f: int(out[f'{t.__name__}.{f}']) for f, *_ in t._fields_}) for t in structs}


def header_text():
    """include/gq.h without its comments"""
    return re.sub(r'/\*.*?\*/', ' ', (ROOT / 'include' / 'gq.h').read_text(), flags=re.S)


def header_constants():
    """{name: value} of the header's `#define GQ_* <integer>` lines (an integer, or a sum / product of integers and earlier names)"""
    out = {}
    for name, text in re.findall(r'^#define (GQ_\w+)[ \t]+(\S.*?)[ \t]*$', header_text(), flags=re.M):
        text = re.sub(r'GQ_\w+', lambda m: str(out.get(m.group(0), m.group(0))), text)
        if re.fullmatch(r'[\d\s()+*-]+', text):
            out[name] = eval(text)   # digits, brackets, + - * only
    return out


def header_prototypes():
    """{name: number of parameters} of every function the header declares"""
    protos = re.findall(r'\b(gq_[a-z_]+)\s*\(([^()]*)\)\s*;', header_text())
    return {name: 0 if params.strip() == 'void' else params.count(',') + 1 for name, params in protos}
