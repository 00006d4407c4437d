"""ctypes binding of libsnake_amd.so (C-ABI declared in include/snake_env.h).

The product has no CPU fallback: if the HIP library is missing or fails to
load, every env constructor raises. Build it with ``python __graft_entry__.py``
(or ``make -C marl-snake_amd/csrc``).
"""
import ctypes
import os

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libsnake_amd.so')

# The header is the one description of the ABI: structs, prototypes and
# constants are read from it (the mapping to ctypes is in _header.py).
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'snake_env.h'))
with open(HEADER_PATH) as _f:
    HEADER = _header.Header(_f.read())
DEFINES = HEADER.defines
EXPORTS = tuple(HEADER.functions)
SNAKE_ABI_VERSION = DEFINES['SNAKE_ABI_VERSION']
ADAM_SCRATCH_BYTES = DEFINES['SNAKE_ADAM_SCRATCH_BYTES']

_S = HEADER.structs
SnakeCfg, SnakeLayout, SnakePaths = _S['snake_cfg'], _S['snake_layout'], _S['snake_paths']
SnakeState, SnakeOut = _S['snake_state'], _S['snake_out']
DqnCfg, DqnLayout, DqnNet, Dqn32Net = (_S['snake_dqn_cfg'], _S['snake_dqn_layout'], _S['snake_dqn_net'],
                                       _S['snake_dqn32_net'])
PolicyCfg, GraphCfg = _S['snake_policy_cfg'], _S['snake_graph_cfg']
ReplayCfg, ReplayLayout, ReplayRings = _S['snake_replay_cfg'], _S['snake_replay_layout'], _S['snake_replay_rings']
GenomeCfg, GenomeProg, GenomeTile, GenomeLayout = (_S['snake_genome_cfg'], _S['snake_genome_prog'],
                                                   _S['snake_genome_tile'], _S['snake_genome_layout'])

ENCODE_PATHS = ('direct', 'rows', 'table', 'lean', 'lean_table')   # SnakePaths.encode


class NativeError(RuntimeError):
    pass


_libs = {}


def lib(path=None):
    """Load libsnake_amd.so once; raise loudly when it is absent. `path` loads an
    alternative build of the same ABI (A/B timing of kernel variants)."""
    path = path or os.environ.get("SNAKE_LIB") or LIB_PATH
    if path in _libs:
        return _libs[path]
    # PyTorch owns device memory and streams: its HIP runtime must be the one in
    # the process before libsnake_amd.so resolves libamdhip64.so.7 (loading ours
    # first brings in /opt/rocm's copy beside torch's, and launches then fail
    # with "no ROCm-capable device").
    import torch  # noqa: F401
    if not os.path.exists(path):
        raise NativeError(f'{path} not built: run `python __graft_entry__.py` '
                          '(hipcc --offload-arch=gfx950); there is no CPU fallback')
    L = ctypes.CDLL(path)
    # (the version first: a library of another ABI may lack a symbol that bind() sets)
    if L.snake_abi_version() != SNAKE_ABI_VERSION:
        raise NativeError('libsnake_amd.so ABI version mismatch; rebuild it')
    HEADER.bind(L)
    _libs[path] = L
    return L


def plan_paths(num_envs, L=None, **kw):
    """snake_plan_paths (include/snake_env.h) as a dict: the kernel variants
    snake_step takes for a SnakeVecEnv(num_envs, **kw). Host only, no device."""
    from .config import build_cfg
    L = L or lib()
    out = SnakePaths()
    check(L.snake_plan_paths(ctypes.byref(build_cfg(**kw)[0]), int(num_envs), ctypes.byref(out)), L)
    return {n: int(getattr(out, n)) for n, _ in SnakePaths._fields_}


def timing_enable(on, L=None):
    check((L or lib()).snake_timing_enable(1 if on else 0), L)


def debug_set(name, value, L=None):
    """snake_debug_set (include/snake_env.h): a process-wide testing knob."""
    check((L or lib()).snake_debug_set(name.encode(), int(value)), L)


def timing_read(kernel, L=None):
    """(total device ms, launches) of one kernel since its last read; for
    kernel='resets' / 'resets_timed' / 'spawn_hits' / 'spawn_jobs' a count (ms is 0)."""
    L = L or lib()
    ms, n = ctypes.c_double(0.0), ctypes.c_int64(0)
    check(L.snake_timing_read(kernel.encode(), ctypes.byref(ms), ctypes.byref(n)), L)
    return ms.value, n.value


def check(rc, L=None):
    if rc < 0:
        msg = (L or lib()).snake_last_error().decode(errors='replace')
        if rc == DEFINES['SNAKE_E_CONFIG']:
            raise ValueError(msg)
        raise NativeError(f'snake C-ABI error {rc}: {msg}')
    return rc
