"""ctypes binding of libsnake_amd.so (C-ABI declared in include/snake_env.h).

The product has no CPU fallback: if the HIP library is missing or fails to
load, every env constructor raises. Build it with ``python __graft_entry__.py``
(or ``make -C marl-snake_amd/csrc``).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libsnake_amd.so')

SNAKE_ABI_VERSION = 20

# Symbols include/snake_env.h declares (checked by tests/test_capi.py).
EXPORTS = ('snake_plan', 'snake_plan_paths', 'snake_build_candidates', 'snake_seed', 'snake_reset', 'snake_step',
           'snake_sync', 'snake_release', 'snake_render_rgb', 'snake_timing_enable', 'snake_timing_read', 'snake_debug_set', 'snake_last_error', 'snake_abi_version',
           'snake_dqn_plan', 'snake_dqn_rows', 'snake_dqn_forward', 'snake_dqn32_scratch', 'snake_dqn32_forward',
           'snake_dqn_map_plan', 'snake_dqn_map_rows', 'snake_dqn_map_forward',
           'snake_policy_plan', 'snake_safe_actions', 'snake_greedy_actions',
           'snake_replay_plan', 'snake_replay_push', 'snake_replay_gather',
           'snake_genome_plan', 'snake_genome_check', 'snake_genome_tiles', 'snake_genome_actions',
           'snake_graph_plan', 'snake_graph_weights', 'snake_graph_obs',
           'snake_dqn32_train_scratch', 'snake_dqn32_backward', 'snake_dqn_td_loss', 'snake_adam_step',
           'snake_dqn_pack32', 'snake_dqn_pack32_host', 'snake_dqn32_backward_bf16',
           'snake_dqn32_forward_bf16_scratch', 'snake_dqn32_forward_bf16',
           'snake_pyrandom_plan', 'snake_pyrandom_act', 'snake_pyrandom_sample')

ADAM_SCRATCH_BYTES = 4112       # SNAKE_ADAM_SCRATCH_BYTES


class SnakeCfg(ctypes.Structure):
    _fields_ = [('height', ctypes.c_int32), ('width', ctypes.c_int32),
                ('num_snakes', ctypes.c_int32), ('snake_length', ctypes.c_int32),
                ('vision_range', ctypes.c_int32), ('frame_stack', ctypes.c_int32),
                ('observer', ctypes.c_int32), ('num_fruits', ctypes.c_int32),
                ('rew_fruit', ctypes.c_double), ('rew_kill', ctypes.c_double),
                ('rew_lose', ctypes.c_double), ('rew_win', ctypes.c_double),
                ('rew_time', ctypes.c_double), ('max_episode_steps', ctypes.c_double),
                ('coop', ctypes.c_int32), ('autoreset', ctypes.c_int32), ('spawn_ahead', ctypes.c_int32),
                ('spawn_background', ctypes.c_int32)]


class SnakeLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        'grid', 'snake', 'body', 'env', 'ctr', 'stats', 'mt', 'cand', 'jscratch', 'spawn', 'resetq',
        'obs', 'rew',
        'done',
        'ep_done', 'rank', 'ep_stats', 'err', 'n_cand')] + [
        ('obs_h', ctypes.c_int32), ('obs_w', ctypes.c_int32), ('obs_c', ctypes.c_int32),
        ('grid_stride', ctypes.c_int32), ('ring_cap', ctypes.c_int32)]


class SnakePaths(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        'encode', 'enc_group', 'units', 'enc_per_wave', 'enc_wpb', 'desc_in_lds', 'fused', 'background',
        'link', 'logic_lanes', 'logic_wpb')]


ENCODE_PATHS = ('direct', 'rows', 'table', 'lean', 'lean_table')   # SnakePaths.encode


class SnakeState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in (
        'grid', 'snake', 'body', 'env', 'ctr', 'stats', 'mt', 'cand', 'jscratch', 'spawn', 'resetq')]


class SnakeOut(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in (
        'obs', 'rew', 'done', 'ep_done', 'rank', 'ep_stats', 'err')]


class DqnCfg(ctypes.Structure):
    _fields_ = [('height', ctypes.c_int32), ('width', ctypes.c_int32), ('channels', ctypes.c_int32),
                ('num_actions', ctypes.c_int32), ('conv_waves', ctypes.c_int32)]


class DqnLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ('conv1_w', 'conv2_w', 'conv3_w', 'fc1_w', 'fc2_w', 'act_per_obs')] + [
        (n, ctypes.c_int32) for n in ('cpad', 'p16', 'k1', 'lds_conv')]


class DqnNet(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in (
        'conv1_w', 'conv2_w', 'conv3_w', 'fc1_w', 'fc2_w', 'conv1_b', 'conv2_b', 'conv3_b', 'fc1_b', 'fc2_b',
        'fc3_w', 'fc3_b')]


class Dqn32Net(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in (
        'conv1_w', 'conv2_w', 'conv3_w', 'fc1_w', 'fc2_w', 'fc3_w', 'conv1_b', 'conv2_b', 'conv3_b', 'fc1_b',
        'fc2_b', 'fc3_b')]


class PolicyCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('obs_h', 'obs_w', 'obs_c', 'num_snakes', 'fill_limit')]


class ReplayCfg(ctypes.Structure):
    _fields_ = [('obs_h', ctypes.c_int32), ('obs_w', ctypes.c_int32), ('obs_c', ctypes.c_int32),
                ('num_snakes', ctypes.c_int32), ('capacity', ctypes.c_int64),
                ('early_death_steps', ctypes.c_int32), ('early_death_penalty', ctypes.c_double)]


class ReplayLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        'state', 'next_state', 'action', 'reward', 'done', 'count', 'scratch')] + [
        ('packed_row', ctypes.c_int32), ('pitch', ctypes.c_int32)]


class ReplayRings(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ('state', 'next_state', 'action', 'reward', 'done', 'count')]


class GenomeCfg(ctypes.Structure):
    _fields_ = [('num_inputs', ctypes.c_int32), ('num_outputs', ctypes.c_int32), ('num_genomes', ctypes.c_int32),
                ('max_nodes', ctypes.c_int32), ('num_nodes', ctypes.c_int64), ('num_links', ctypes.c_int64)]


class GenomeProg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in (
        'node_off', 'node_act', 'node_bias', 'node_resp', 'link_off', 'link_src', 'link_w', 'out_slot')]


class GenomeTile(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('genome', 'count', 'row_start', 'scratch')]


class GenomeLayout(ctypes.Structure):
    _fields_ = [('scratch', ctypes.c_int64), ('max_tiles', ctypes.c_int64), ('tile_rows', ctypes.c_int32),
                ('lds_nodes', ctypes.c_int32), ('lds_bytes', ctypes.c_int32)]


class GraphCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('obs_h', 'obs_w', 'obs_c', 'num_snakes', 'vision_range', 'source',
                                              'out_f32')]


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
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    L.snake_abi_version.restype = ctypes.c_int
    L.snake_last_error.restype = ctypes.c_char_p
    L.snake_plan.argtypes = [ctypes.POINTER(SnakeCfg), I64, ctypes.POINTER(SnakeLayout)]
    L.snake_plan_paths.argtypes = [ctypes.POINTER(SnakeCfg), I64, ctypes.POINTER(SnakePaths)]
    L.snake_build_candidates.restype = I64
    L.snake_build_candidates.argtypes = [ctypes.POINTER(SnakeCfg), P, I64]
    L.snake_seed.argtypes = [ctypes.POINTER(SnakeCfg), ctypes.POINTER(SnakeState), I64,
                             ctypes.c_uint32, I64, P]
    L.snake_reset.argtypes = [ctypes.POINTER(SnakeCfg), ctypes.POINTER(SnakeState), I64, P,
                              ctypes.POINTER(SnakeOut), P]
    L.snake_step.argtypes = [ctypes.POINTER(SnakeCfg), ctypes.POINTER(SnakeState), I64, P,
                             ctypes.POINTER(SnakeOut), P]
    L.snake_sync.argtypes = [ctypes.POINTER(SnakeCfg), ctypes.POINTER(SnakeState), I64, P]
    L.snake_release.argtypes = [ctypes.POINTER(SnakeCfg), ctypes.POINTER(SnakeState), I64]
    L.snake_render_rgb.argtypes = [ctypes.POINTER(SnakeCfg), ctypes.POINTER(SnakeState), I64, P, P, P]
    L.snake_dqn_plan.argtypes = [ctypes.POINTER(DqnCfg), ctypes.POINTER(DqnLayout)]
    L.snake_dqn_rows.argtypes = [ctypes.POINTER(DqnCfg), P, I64]
    L.snake_dqn_rows.restype = I64
    L.snake_dqn_forward.argtypes = [ctypes.POINTER(DqnCfg), ctypes.POINTER(DqnNet), P, I64, P, P, P, P]
    L.snake_dqn_map_plan.argtypes = L.snake_dqn_plan.argtypes
    L.snake_dqn_map_rows.argtypes = L.snake_dqn_rows.argtypes
    L.snake_dqn_map_rows.restype = I64
    L.snake_dqn_map_forward.argtypes = L.snake_dqn_forward.argtypes
    L.snake_dqn32_scratch.argtypes = [ctypes.POINTER(DqnCfg), I64]
    L.snake_dqn32_scratch.restype = I64
    L.snake_dqn32_forward.argtypes = [ctypes.POINTER(DqnCfg), ctypes.POINTER(Dqn32Net), P, I64, P, P, P, P]
    L.snake_dqn32_train_scratch.argtypes = [ctypes.POINTER(DqnCfg), I64]
    L.snake_dqn32_train_scratch.restype = I64
    L.snake_dqn32_backward.argtypes = [ctypes.POINTER(DqnCfg), ctypes.POINTER(Dqn32Net), P, I64, P, P, P,
                                       ctypes.POINTER(Dqn32Net), P]
    L.snake_dqn32_backward_bf16.argtypes = L.snake_dqn32_backward.argtypes
    L.snake_dqn32_forward_bf16_scratch.argtypes = L.snake_dqn32_scratch.argtypes
    L.snake_dqn32_forward_bf16_scratch.restype = I64
    L.snake_dqn32_forward_bf16.argtypes = L.snake_dqn32_forward.argtypes
    F32 = ctypes.c_float
    L.snake_dqn_td_loss.argtypes = [P, P, P, P, P, I64, ctypes.c_int32, F32, P, P, P, P]
    L.snake_adam_step.argtypes = [P, P, P, P, I64, I64, F32, F32, F32, F32, F32, P, P, P]
    L.snake_dqn_pack32.argtypes = [ctypes.POINTER(DqnCfg), ctypes.c_int32, ctypes.POINTER(Dqn32Net),
                                   ctypes.POINTER(DqnNet), P, P]
    L.snake_dqn_pack32_host.argtypes = L.snake_dqn_pack32.argtypes[:5]
    L.snake_policy_plan.argtypes = [ctypes.POINTER(PolicyCfg)]
    L.snake_safe_actions.argtypes = [ctypes.POINTER(PolicyCfg), P, P, P, P, P, I64, P]
    L.snake_greedy_actions.argtypes = [ctypes.POINTER(PolicyCfg), P, P, P, P, P, I64, P]
    L.snake_replay_plan.argtypes = [ctypes.POINTER(ReplayCfg), I64, ctypes.POINTER(ReplayLayout)]
    L.snake_replay_push.argtypes = [ctypes.POINTER(ReplayCfg), ctypes.POINTER(ReplayRings), P, P, P, P, P, P, P,
                                    I64, P, P]
    L.snake_replay_gather.argtypes = [ctypes.POINTER(ReplayCfg), ctypes.POINTER(ReplayRings), P, I64,
                                      ctypes.c_int32, P, P, P, P, P, P]
    L.snake_pyrandom_plan.argtypes = [ctypes.c_int32, I64, I64]
    L.snake_pyrandom_act.argtypes = [P, P, ctypes.c_double, P, P, P, P, I64, ctypes.c_int32, ctypes.c_int32, P]
    L.snake_pyrandom_sample.argtypes = [P, P, I64, P, I64, I64, P, P, P]
    L.snake_genome_plan.argtypes = [ctypes.POINTER(GenomeCfg), I64, ctypes.POINTER(GenomeLayout)]
    L.snake_genome_check.argtypes = [ctypes.POINTER(GenomeCfg), ctypes.POINTER(GenomeProg)]
    L.snake_genome_tiles.argtypes = [ctypes.POINTER(GenomeCfg), P, P, I64, ctypes.c_int32, P, P, I64]
    L.snake_genome_tiles.restype = I64
    L.snake_genome_actions.argtypes = [ctypes.POINTER(GenomeCfg), ctypes.POINTER(GenomeProg), P, P, I64, P, P, P, P,
                                       P, I64, P]
    L.snake_graph_plan.argtypes = [ctypes.POINTER(GraphCfg)]
    L.snake_graph_weights.argtypes = [ctypes.c_int32, ctypes.c_int32, P]
    L.snake_graph_obs.argtypes = [ctypes.POINTER(GraphCfg), P, P, P, I64, P]
    L.snake_timing_enable.argtypes = [ctypes.c_int]
    L.snake_debug_set.argtypes = [ctypes.c_char_p, ctypes.c_longlong]
    L.snake_timing_read.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                    ctypes.POINTER(ctypes.c_int64)]
    if L.snake_abi_version() != SNAKE_ABI_VERSION:
        raise NativeError('libsnake_amd.so ABI version mismatch; rebuild it')
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
        if rc == -1:
            raise ValueError(msg)
        raise NativeError(f'snake C-ABI error {rc}: {msg}')
    return rc
