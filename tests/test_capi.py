"""CPU checks of the product's C-ABI library (no GPU needed): it loads, exports
every symbol include/snake_env.h declares, plans buffers, rejects bad configs
the way SnakeEnv.__init__ does, and its host-side spawn-pose table equals the
reference's dfs_sweep_empty order (golden digests)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import golden_io as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def native():
    from marlenv import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native


def header_functions():
    src = open(os.path.join(ROOT, 'include', 'snake_env.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'^\s*(?:const\s+)?\w+\s*\*?\s*(snake_\w+)\s*\(', src, flags=re.M)))


def test_exports_match_header(native):
    names = header_functions()
    assert set(names) == set(native.EXPORTS), names
    L = native.lib()
    for n in names:
        assert hasattr(L, n), n
    assert L.snake_abi_version() == native.SNAKE_ABI_VERSION


def test_struct_layouts_match_the_c_compiler(native, tmp_path):
    """The Structures read from the header have the sizes and field offsets a C
    compiler gives the header's own structs: one _Static_assert per struct and
    per field."""
    lines = ['#include <stddef.h>', '#include "snake_env.h"']
    for name, T in native.HEADER.structs.items():
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(T)}, "sizeof {name}");')
        lines += [f'_Static_assert(offsetof({name}, {f}) == {getattr(T, f).offset}, "{name}.{f}");'
                  for f, _ in T._fields_]
    assert len(native.HEADER.structs) >= 19 and len(lines) >= 2 + 190
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines) + '\n')
    rocm_clang = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin', 'clang')
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or rocm_clang
    r = subprocess.run([cc, '-std=c11', '-fsyntax-only', '-I' + os.path.join(ROOT, 'include'), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_every_function_is_bound(native):
    """Every prototype of the header, found by a regex of this test's own, is bound
    on the loaded library with as many argtypes as the header has arguments and
    the restype of its return type."""
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'snake_env.h')).read(), flags=re.S)
    protos = re.findall(r'^(int|int64_t|const char \*)\s*(snake_\w+)\(([^)]*)\);', src, flags=re.M)
    assert [n for _, n, _ in protos] == list(native.EXPORTS) and len(protos) == len(header_functions())
    restypes = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'const char *': ctypes.c_char_p}
    L = native.lib()
    for ret, name, args in protos:
        f = getattr(L, name)
        assert len(f.argtypes) == (0 if args.strip() == 'void' else args.count(',') + 1), name
        assert f.restype is restypes[ret], name
    assert L.snake_step.argtypes[:2] == [ctypes.POINTER(native.SnakeCfg), ctypes.POINTER(native.SnakeState)]
    # snake_genome_tile and snake_epi_stat are passed as raw addresses
    assert L.snake_genome_actions.argtypes[2] is ctypes.c_void_p
    assert dict(native.SnakeState._fields_)['stats'] is ctypes.c_void_p


SHORT_HEADER = """\
/* a comment; with { and ( in it */
#ifdef __cplusplus
extern "C" {
#endif
#define SNAKE_TWO 2          // two; {
#define SNAKE_NEG (-128)
#define SNAKE_HEX 0x10
#define SNAKE_GUARD
typedef struct {
    int32_t height, width;   /* both; in cells */
    double  scale;
    uint16_t fruits, kills;
    const float *w, *b;      // pointers (two)
    int64_t *count;
} snake_a;
typedef struct { snake_a *a; const snake_epi_stat *stats; uint8_t flag; } snake_b;
int snake_f(const snake_a *a, int64_t n,
            snake_b *out,   /* written; */
            void *stream);
int snake_void(void);
int snake_ll(const char *name, long long value, float x, snake_epi_stat *s);
const char *snake_text(void);
int64_t snake_count(const int32_t *rows);
#ifdef __cplusplus
}
#endif
"""


def test_header_parser():
    from marlenv._header import Header
    c = ctypes
    h = Header('typedef struct { double score; } snake_epi_stat;\n' + SHORT_HEADER)
    assert h.defines == {'SNAKE_TWO': 2, 'SNAKE_NEG': -128, 'SNAKE_HEX': 16}
    A, B = h.structs['snake_a'], h.structs['snake_b']
    assert A._fields_ == [('height', c.c_int32), ('width', c.c_int32), ('scale', c.c_double),
                          ('fruits', c.c_uint16), ('kills', c.c_uint16), ('w', c.c_void_p), ('b', c.c_void_p),
                          ('count', c.c_void_p)]
    assert B._fields_ == [('a', c.POINTER(A)), ('stats', c.c_void_p), ('flag', c.c_uint8)]
    assert list(h.functions) == ['snake_f', 'snake_void', 'snake_ll', 'snake_text', 'snake_count']
    assert h.functions['snake_f'] == (c.c_int, [c.POINTER(A), c.c_int64, c.POINTER(B), c.c_void_p])
    assert h.functions['snake_void'] == (c.c_int, [])
    assert h.functions['snake_ll'] == (c.c_int, [c.c_char_p, c.c_longlong, c.c_float, c.c_void_p])
    assert h.functions['snake_text'] == (c.c_char_p, [])
    assert h.functions['snake_count'] == (c.c_int64, [c.c_void_p])


@pytest.mark.parametrize('text,line,word', [
    ('int snake_ok(void);\n\n/* two\n lines */ int snake_f(size_t n);\n', 4, 'size_t'),      # unknown type, argument
    ('typedef struct {\n    int32_t a;\n    unsigned b;\n} snake_s;\n', 3, 'unsigned'),       # unknown type, field
    ('snake_t snake_f(void);\n', 1, 'snake_t'),                                               # unknown type, return
    ('typedef struct {\n    int32_t a\n} snake_s;\n', 2, 'int32_t a'),                        # no ';'
    ('int snake_ok(void);\nint snake_f(int (*cb)(int));\n', 2, 'snake_f'),                    # not read
    ('int snake_f(int32_t);\n', 1, 'int32_t'),                                                # an argument without a name
    ('int snake_f(void x);\n', 1, 'void'),
    ('#define SNAKE_OK 0\n#define SNAKE_X (1 << 3)\n', 2, 'SNAKE_X'),                        # a define that is no literal
    ('#define SNAKE_MAX(a, b) 4\n', 1, 'SNAKE_MAX'),
])
def test_header_parser_names_the_line_it_cannot_read(text, line, word):
    from marlenv._header import Header, HeaderError
    with pytest.raises(HeaderError, match=rf'^line {line}: .*{word}'):
        Header(text)


def cfg(native, **kw):
    from marlenv.config import build_cfg
    return build_cfg(**kw)[0]


def test_plan_sizes(native):
    c = cfg(native, height=20, width=20, num_snakes=4, vision_range=5)
    lay = native.SnakeLayout()
    assert native.lib().snake_plan(ctypes.byref(c), 65536, ctypes.byref(lay)) == 0
    assert (lay.obs_h, lay.obs_w, lay.obs_c) == (11, 11, 8)
    assert lay.obs == 65536 * 4 * 11 * 11 * 8
    assert lay.n_cand == 3464 and lay.jscratch == 0
    assert lay.grid_stride == 400 and lay.ring_cap == 512
    assert lay.spawn == 65536 * 672 * 4                        # spawn-ahead records
    assert lay.stats == 65536 * 4 * 16                         # snake_epi_stat: one 16-B record per snake
    # four queue sets (kQSets) of three queues + counters (one per 128-B line),
    # then the fused step's counts, flags and hand-off records
    queues = 4 * (3 * 64 * (4096 // 64) * 16 + 227 * 32)   # (four queue sets)
    assert lay.resetq == (queues + 64 * 32 + 2 * 65536 // 4 + 4 * 65536) * 4
    c = cfg(native, height=40, width=40, num_snakes=8, vision_range=5, frame_stack=4)
    assert native.lib().snake_plan(ctypes.byref(c), 8192, ctypes.byref(lay)) == 0
    assert lay.obs_c == 32 and lay.obs == 8192 * 8 * 11 * 11 * 32
    # the u16 draw record fits LDS (the spawn kernel keeps it there), and with
    # background spawn-ahead the one-launch workers (k_post_lean) keep a global
    # link table per worker for resets without a ready record
    assert lay.n_cand == 16424 and lay.jscratch == 2048 * (16424 + 64) * 4
    assert lay.spawn == 4 * 8192 * 672 * 4                        # background spawn-ahead: a record per queue set and env
    c = cfg(native, height=44, width=44, num_snakes=4)
    lay2 = native.SnakeLayout()
    assert native.lib().snake_plan(ctypes.byref(c), 8192, ctypes.byref(lay2)) == 0
    assert lay2.n_cand == 20168 and lay2.jscratch == 2048 * (20168 + 64) * 4   # global link tables
    assert lay.grid == 8192 * 4 * 1600
    # every-step / no auto-reset: the 40x40 four-frame board needs no worker link tables
    for kw in (dict(autoreset=False), dict(autoreset='every_step')):
        c = cfg(native, height=40, width=40, num_snakes=8, vision_range=5, frame_stack=4, **kw)
        assert native.lib().snake_plan(ctypes.byref(c), 64, ctypes.byref(lay)) == 0
        assert lay.jscratch == 0 and lay.spawn == 64 * 672 * 4, kw
    # in-step spawn-ahead on that board (spawn_background=-1): one record per env,
    # the k_post_lean workers' link tables
    c = cfg(native, height=40, width=40, num_snakes=8, vision_range=5, frame_stack=4, spawn_background=-1)
    assert native.lib().snake_plan(ctypes.byref(c), 64, ctypes.byref(lay)) == 0
    assert lay.jscratch == 64 * (16424 + 64) * 4 and lay.spawn == 64 * 672 * 4


@pytest.mark.parametrize('kw,N,bg', [
    (dict(height=20, width=20), 4096, True),                     # cfg2: 50 MiB of obs per step
    (dict(height=20, width=20), 8192, False),                    # 100 MiB
    (dict(height=20, width=20, vision_range=5), 8192, True),     # cfg3's board at 8 192 envs
    (dict(height=20, width=20, vision_range=5), 16384, False),   # more than 8 192 envs
    (dict(height=20, width=20, spawn_background=-1), 4096, False),
    (dict(height=20, width=20, spawn_ahead=-1), 1024, False),    # nothing to draw ahead
])
def test_plan_background_automatic(native, kw, N, bg):
    """spawn_background = 0 (automatic) turns the background spawn kernel on for
    batches of at most 8 192 envs and 64 MiB of observations per step (round 5):
    the layout then holds a spawn-ahead record per queue set (four) and env."""
    c = cfg(native, num_snakes=4, **kw)
    lay = native.SnakeLayout()
    assert native.lib().snake_plan(ctypes.byref(c), N, ctypes.byref(lay)) == 0
    assert lay.spawn == (4 if bg else 1) * N * 672 * 4, (kw, N)


@pytest.mark.parametrize('H,W,L,N', [(50, 50, 3, 16384), (72, 72, 3, 4096), (100, 100, 2, 65536)])
def test_plan_large_boards(native, H, W, L, N):
    """Boards whose k_logic frames do not fit four waves per workgroup (ADVICE r4:
    4 x 41 KB at 50x50 and 16 envs per wave) still plan: snake_plan runs the
    launch-side checks too (build_kcfg's plan_logic), which pick one wave per workgroup or
    fewer envs per wave instead of a launch that fails."""
    c = cfg(native, height=H, width=W, snake_length=L, num_snakes=4, vision_range=3)
    lay = native.SnakeLayout()
    assert native.lib().snake_plan(ctypes.byref(c), N, ctypes.byref(lay)) == 0, \
        native.lib().snake_last_error().decode()


@pytest.mark.parametrize('kw,msg', [
    (dict(num_snakes=0), 'num_snakes'), (dict(num_snakes=17), 'num_snakes'),
    (dict(snake_length=1), 'snake_length'), (dict(height=2), 'height'),
    (dict(num_fruits=0), 'num_fruits'), (dict(frame_stack=0), 'frame_stack'),
    (dict(height=5, width=5, num_snakes=4, snake_length=3), 'too small'),
    # 61 interior cells for 60 snake cells: ~1e-5 of the spawn draws are disjoint
    (dict(height=3, width=63, num_snakes=4, snake_length=15), 'too crowded'),
])
def test_plan_rejects(native, kw, msg):
    c = cfg(native, **kw)
    lay = native.SnakeLayout()
    rc = native.lib().snake_plan(ctypes.byref(c), 16, ctypes.byref(lay))
    assert rc == -1
    assert msg in native.lib().snake_last_error().decode()
    with pytest.raises(ValueError):
        native.check(rc)


def test_reward_dict_keys_are_checked(native):
    from marlenv.config import build_cfg
    with pytest.raises(KeyError):                   # snake_env.py:77-80
        build_cfg(reward_dict={'fruit': 1.0})
    c, meta = build_cfg(num_snakes=4)
    assert meta['num_fruits'] == 3                  # int(round(0.8 * 4))
    assert build_cfg(num_snakes=1)[1]['num_fruits'] == 1


def table(native, H, W, L):
    c = cfg(native, height=H, width=W, snake_length=L, num_snakes=1)
    n = native.lib().snake_build_candidates(ctypes.byref(c), None, 0)
    out = np.zeros(n * L, np.int16)
    assert native.lib().snake_build_candidates(ctypes.byref(c), out.ctypes.data_as(ctypes.c_void_p), out.size) == n
    cells = out.reshape(n, L).astype(np.int64)
    return np.stack([cells // W, cells % W], -1).astype(np.int16)


def test_spawn_table_matches_reference(native):
    z = G.load('candidates.npz')
    for k in z.files:
        if k.startswith('full_'):
            H, W = map(int, k.split('_')[1].split('x'))
            L = int(k.split('_L')[1])
            np.testing.assert_array_equal(table(native, H, W, L), z[k])
    for H, W, L, C, dg in z['digest_meta']:
        t = table(native, int(H), int(W), int(L))
        assert t.shape[0] == int(C) and G.digest(t) == int(dg)


def test_kernarg_pointer_only_at_kernel_entry():
    """The kernarg-segment builtin means the running kernel's arguments only in
    the kernel itself: it occurs once, in kernel_args(), and kernel_args() is
    called only as the first statement of a __global__ function (device
    functions take the pointer as an argument, inlined or not)."""
    d = os.path.join(ROOT, 'marl-snake_amd', 'csrc')
    src = '\n'.join(re.sub(r'//[^\n]*', '', open(os.path.join(d, f)).read()) for f in sorted(os.listdir(d)))
    assert len(re.findall(r'KPtr kernel_args\(\)\s*\{[^}]*__builtin_amdgcn_kernarg_segment_ptr\(\)[^}]*\}', src)) == 1
    assert src.count('__builtin_amdgcn_kernarg_segment_ptr') == 1
    calls = len(re.findall(r'kernel_args\(\)', src)) - 1   # (less the definition)
    entries = re.findall(r'__global__[^{;]*\{\s*const KPtr kp = kernel_args\(\);', src)
    assert calls == len(entries) == 7
