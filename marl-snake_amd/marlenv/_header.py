"""Reads a C header of plain declarations (include/snake_env.h) into ctypes:
every `typedef struct { ... } name;` as a Structure, every prototype as
(restype, argtypes), every `#define SNAKE_* <integer>` as an int.

    fixed-width integers, int, long long, float, double   their ctypes
    const char *                                          c_char_p
    pointer to a struct of the header                     POINTER(that struct)
    any other pointer                                     c_void_p

A declaration that does not read, a type name that is not known, or a SNAKE_*
define whose value is not an integer literal (one without a value, like the
include guard, is skipped) raises HeaderError with its line: nothing is guessed.
"""
import ctypes
import re

SCALARS = {'void': None, 'char': ctypes.c_char, 'int': ctypes.c_int, 'long long': ctypes.c_longlong,
           'float': ctypes.c_float, 'double': ctypes.c_double,
           **{f'{u}int{n}_t': getattr(ctypes, f'c_{u}int{n}') for u in ('', 'u') for n in (8, 16, 32, 64)}}
# These two live in device or array memory: callers pass their raw addresses.
RAW_ADDRESS = {'snake_epi_stat', 'snake_genome_tile'}

_DECL = re.compile(r'\s*(?:typedef\s+struct\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)'
                   r'|(?P<ret>[\w\s*]+?\b\w+)\s*\((?P<args>[^()]*)\))\s*;')
_TYPE = re.compile(r'\s*(?:const\s+)?(long\s+long|\w+)\b')
_DEFINE = re.compile(r'^[ \t]*#[ \t]*define[ \t]+(SNAKE_\w+)\b[ \t]*(.*?)[ \t]*$', re.M)
_INTEGER = re.compile(r'\(?\s*(-?(?:0[xX][0-9a-fA-F]+|\d+))\s*\)?')


class HeaderError(ValueError):
    pass


def _blank(m):
    return '\n' * m.group(0).count('\n')


class Header:
    def __init__(self, text):
        self.structs, self.functions, self.defines = {}, {}, {}
        # (comments first: they hold ';', '{' and parentheses; newlines stay, for the line numbers)
        self.text = text = re.sub(r'/\*.*?\*/|//[^\n]*', _blank, text, flags=re.S)
        for m in _DEFINE.finditer(text):
            if m[2]:
                value = _INTEGER.fullmatch(m[2]) or self.fail(m.start(), 'not an integer literal')
                self.defines[m[1]] = int(value[1], 0)
        text = re.sub(r'#\s*ifdef\s+__cplusplus.*?#\s*endif', _blank, text, flags=re.S)
        self.text = text = re.sub(r'^[ \t]*#[^\n]*', '', text, flags=re.M)
        pos = 0
        while text[pos:].strip():
            m = _DECL.match(text, pos) or self.fail(pos, 'cannot read the declaration')
            if m['struct']:
                *fields, (at, tail) = self.pieces(m, 'body', ';')
                if tail.strip():
                    self.fail(at, "missing ';'")
                fields = [f for at, decl in fields for f in self.declarators(decl, at)]
                self.structs[m['struct']] = type(m['struct'], (ctypes.Structure,), {'_fields_': fields})
            else:
                (name, restype), = self.declarators(m['ret'], m.start('ret'), void=True)
                args = [] if m['args'].strip() == 'void' else [
                    t for at, decl in self.pieces(m, 'args', ',') for _, t in self.declarators(decl, at)]
                self.functions[name] = (restype, args)
            pos = m.end()

    def fail(self, pos, what):
        pos += len(self.text[pos:]) - len(self.text[pos:].lstrip())
        line = self.text.count('\n', 0, pos) + 1
        raise HeaderError(f'line {line}: {what}: {self.text[pos:].splitlines()[0].strip()!r}')

    @staticmethod
    def pieces(m, group, sep):
        """(position, text) of the pieces of a match's group between its `sep`s."""
        at = m.start(group)
        for p in m[group].split(sep):
            yield at, p
            at += len(p) + 1

    def declarators(self, decl, at, void=False):
        """[(name, ctype)] of `type a, *b`: a struct's field line, one argument, or `ret function`."""
        t = _TYPE.match(decl)
        names = [re.fullmatch(r'([\s*]*)\b(\w+)\s*', d) for d in decl[t.end():].split(',')] if t else [None]
        if not all(names):
            self.fail(at, 'cannot read the declaration')
        out = [(n[2], self.ctype(' '.join(t[1].split()), n[1].count('*'), at)) for n in names]
        if not void and any(c is None for _, c in out):
            self.fail(at, 'a void value')
        return out

    def ctype(self, base, stars, at):
        if base not in SCALARS and base not in self.structs:
            self.fail(at, f'unknown type {base!r}')
        if stars == 0:
            return SCALARS[base] if base in SCALARS else self.structs[base]
        if stars == 1 and base == 'char':
            return ctypes.c_char_p
        if stars == 1 and base in self.structs and base not in RAW_ADDRESS:
            return ctypes.POINTER(self.structs[base])
        return ctypes.c_void_p

    def bind(self, library):
        """Sets restype and argtypes of every prototype on a loaded library."""
        for name, (restype, argtypes) in self.functions.items():
            f = getattr(library, name)
            f.restype, f.argtypes = restype, argtypes
