// step_encode.h -- the observation encodes: the observation stores, the direct,
// lean and row-wise encodes of one env (encode, encode_lean, encode_rows), and
// the per-wave drivers of k_encode / k_post / k_post_lean / k_step (encode_one,
// encode_multi, the table encode encode_tbl_block, encode_lean_block).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "snake_internal.h"
#include "step_args.h"
#include "step_lanes.h"

namespace snake {

// Observation stores (the step's bulk output, 2/3 of its bytes) as
// non-temporal stores: streamed past the caches, so they do not evict the env
// state the next step's k_logic reads (cfg3 0.0929 -> 0.0908 ms, round 3).
// (Round 5: write-back stores measured slower in the step -- cfg3 0.0846 ->
// 0.0887 ms, cfg5 0.1019 -> 0.1184 -- although a lone store stream reaches
// 5.3 TB/s with them against 4.5 TB/s non-temporal, scripts/microbench/storebw.hip.)
template <typename T>
__device__ __forceinline__ void obs_store(T *p, const T &v)
{
    __builtin_nontemporal_store(v, p);
}
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));

// The table encode's observation stores as raw buffer stores on the env's
// observation (a wave-uniform descriptor: no 64-bit address per store) with an
// explicit cache policy: non-temporal (as obs_store). Round 6 measured the
// others, same box, ms per step, not kept: sc1 (write-through, policy 16; 17 =
// sc0 sc1) would leave no dirty lines for the kernel-end writeback but was slower
// (cfg3 0.0821 -> 0.0985, cfg5 0.0812 -> 0.0982, cfg4 0.0546 -> 0.0570; cfg3s8
// 0.0390 -> 0.0387); the buffer form itself, non-temporal, is kept: cfg4
// 0.0556 -> 0.0549, cfg3 and the driver window equal (profiles/r06_ab_obs_policy.txt).
__device__ __forceinline__ void obs_store_rs(__amdgpu_buffer_rsrc_t rs, int byte_off, v4u v)
{
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, byte_off, 0, 2);   // (nt)
}

// (Round 6: storing the two 128-byte lines an env's observation shares with
// its neighbours write-back, the rest non-temporal, measured slower in the step
// -- the per-store edge test in the encodes' store loops cost more than the
// merged lines saved: cfg3 0.0830 -> 0.0848 ms, driver window 0.0866 -> 0.0915,
// cfg5 k_post_lean 57 -> 75 us; profiles/r06_ab_edge_removed.txt.)

// The encode waves' priority beside the reset workers (KCfg.encode_prio; 0
// leaves it as launched).
__device__ __forceinline__ void encode_setprio(const KCfg &c)
{
    if (c.encode_prio == 1) __builtin_amdgcn_s_setprio(1);      // (setprio takes an immediate)
    else if (c.encode_prio == 2) __builtin_amdgcn_s_setprio(2);
    else if (c.encode_prio == 3) __builtin_amdgcn_s_setprio(3);
}

// ------------------------------------------------------------------ encode
// _encode (snake_env.py:474-519) + frame stack (:444-472): for snake k the 8
// channels [wall, fruit, other head/body/tail, own head/body/tail]; with a vision
// range the (2vr+1)^2 window is centred on the own-HEAD cell (argmax of the own
// head plane: the snake's head while alive, (0,0) once dead) and zero outside
// the grid. org[f*16+k] = crop origin of snake k in frame f, packed
// ((r0 + 256) << 16) | (c0 + 256).
__device__ __forceinline__ unsigned long long onehot(int v, int k)
{
    const int id = div10(v);
    const int code = v - 10 * id;                   // 3 HEAD, 4 BODY, 5 TAIL
    const int ch = (v < 3) ? v - 1 : ((id == k) ? code + 2 : code - 1);
    return v == C_EMPTY ? 0ull : (1ull << (8 * ch));
}

__device__ __forceinline__ unsigned long long unit_bits(const KCfg &c, const uint8_t *frames,
                                                       const int *org, int k, int i, int j, int s)
{
    const int p = org[s * kMaxSnakes + k];
    const int r = (p >> 16) - 256 + i, cc = (p & 0xffff) - 256 + j;
    if ((unsigned)r >= (unsigned)c.H || (unsigned)cc >= (unsigned)c.W) return 0ull;
    return onehot(frames[s * c.grid_stride + r * c.W + cc], k);
}

// obs layout (S, oh, ow, 8*fs): unit u = ((k*oh + i)*ow + j)*fs + f is 8 bytes;
// frame f (oldest first) is ring slot (slot0 + f) % fs of the LDS ring.
// Lane l writes units 2l, 2l+1 (16 bytes) then strides by 128 units; the
// (k,i,j,f) digits advance by carries, no division in the loop.
__device__ void encode(const KCfg &c, const uint8_t *frames, const int *org, int slot0,
                       uint8_t *obs_env, int lane)
{
    const int U = c.units, pairs = (U + 1) >> 1, fs = c.fs;
    int u = 2 * lane;
    int f = u % fs, rest = u / fs;
    int j = rest % c.ow;
    rest /= c.ow;
    int i = rest % c.oh;
    int k = rest / c.oh;
    const bool wide = (U & 1) == 0;
    for (int p = lane; p < pairs; p += kWave) {
        int s = slot0 + f;
        s -= (s >= fs) ? fs : 0;
        const unsigned long long a = unit_bits(c, frames, org, k, i, j, s);
        int f2 = f + 1, j2 = j, i2 = i, k2 = k;
        if (f2 == fs) {
            f2 = 0;
            if (++j2 == c.ow) { j2 = 0; if (++i2 == c.oh) { i2 = 0; k2++; } }
        }
        int s2 = slot0 + f2;
        s2 -= (s2 >= fs) ? fs : 0;
        const bool has_b = 2 * p + 1 < U;
        const unsigned long long b = has_b ? unit_bits(c, frames, org, k2, i2, j2, s2) : 0ull;
        if (wide) {
            uint4 v;
            v.x = (uint32_t)a; v.y = (uint32_t)(a >> 32);
            v.z = (uint32_t)b; v.w = (uint32_t)(b >> 32);
            obs_store(reinterpret_cast<v4u *>(obs_env + 16 * (int64_t)p), (v4u){v.x, v.y, v.z, v.w});
        } else {
            obs_store(reinterpret_cast<unsigned long long *>(obs_env + 16 * (int64_t)p), a);
            if (has_b) obs_store(reinterpret_cast<unsigned long long *>(obs_env + 16 * (int64_t)p + 8), b);
        }
        f += c.adv_f;
        if (f >= fs) { f -= fs; j++; }
        j += c.adv_j;
        if (j >= c.ow) { j -= c.ow; i++; }
        i += c.adv_i;
        if (i >= c.oh) { i -= c.oh; k++; }
        k += c.adv_k;
    }
}

// Lean encode (k_encode): the observation straight from a zero-bordered copy
// of the env's frames in LDS (pf: frame s's grid cell (r, c) at s*pframe +
// (r + vr)*pw + c + lp, zero around it), so a crop window never needs a bounds
// test; base[s*16 + k] = the LDS offset of snake k's window origin in frame s
// (0 for the full map). Lane = one 16-byte output chunk = two consecutive
// units (8 obs bytes each: one cell of one frame): per unit one LDS byte read
// and its one-hot channel (_encode :481-492), no LDS staging of the output, no
// divergent branch.
template <int T = kWave>
__device__ void encode_lean(const KCfg &c, const uint8_t *pf, const int *base, int slot0, uint8_t *obs_env,
                            int lane)
{
    const int pairs = c.units >> 1;
    for (int p = lane; p < pairs; p += T) {
        const uint32_t u = 2u * (uint32_t)p;
        int kk = (int)__umulhi(u, c.mag_ups);
        const int r0 = (int)u - kk * c.ups;
        int ii = (int)__umulhi((uint32_t)r0, c.mag_rowl);
        const int r1 = r0 - ii * c.rowl;
        int jj = fdiv((uint32_t)r1, c.mag_fs, c.fs);
        int ff = r1 - jj * c.fs;
        uint32_t w[4];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            int s = slot0 + ff;
            s -= (s >= c.fs) ? c.fs : 0;
            const int v = pf[s * c.pframe + base[s * kMaxSnakes + kk] + ii * c.pw + jj];
            const int id = div10(v), code = v - 10 * id;
            const int ch = (v < 3) ? v - 1 : ((id == kk) ? code + 2 : code - 1);
            const uint32_t bit = (v != 0) ? (1u << (8 * (ch & 3))) : 0u;
            w[2 * h] = ch < 4 ? bit : 0u;
            w[2 * h + 1] = ch < 4 ? 0u : bit;
            if (h == 0) {   // the next unit: frame, then column, row, snake digits carry
                ff++;
                const bool cf = ff == c.fs;
                ff = cf ? 0 : ff;
                jj += cf;
                const bool cj = jj == c.ow;
                jj = cj ? 0 : jj;
                ii += cj;
                const bool ci = ii == c.oh;
                ii = ci ? 0 : ii;
                kk += ci;
            }
        }
        obs_store(reinterpret_cast<v4u *>(obs_env) + p, (v4u){w[0], w[1], w[2], w[3]});
    }
}

// env e's frames into the zero-bordered LDS image of encode_lean (the border
// was zeroed by the caller and is never written) and its window origins.
__device__ void stage_lean(const KCfg &c, const snake_state &st, int64_t e, uint8_t *pf, int *base, int lane)
{
    const uint8_t *ring = st.grid + e * c.ring_bytes;
    const int tp = c.vr;
    if ((c.W & 3) == 0) {
        const int wpr = c.W >> 2, nw = c.H * wpr;
        const uint32_t *r32 = reinterpret_cast<const uint32_t *>(ring);
        uint32_t *p32 = reinterpret_cast<uint32_t *>(pf);
        for (int s = 0; s < c.fs; s++)
            for (int x = lane; x < nw; x += kWave) {
                const int r = fdiv((uint32_t)x, c.mag_wpr, wpr), c4 = x - r * wpr;
                p32[(s * c.pframe + (r + tp) * c.pw + c.lp) / 4 + c4] = r32[s * (c.grid_stride >> 2) + x];
            }
    } else {
        for (int s = 0; s < c.fs; s++)
            for (int x = lane; x < c.HW; x += kWave) {
                const int r = (int)__umulhi((uint32_t)x, c.mag_W), cc = x - r * c.W;
                pf[s * c.pframe + (r + tp) * c.pw + c.lp + cc] = ring[s * c.grid_stride + x];
            }
    }
    const int fsS = c.fs * c.S;
    if (lane < fsS) {
        const int x = lane / c.S, k = lane - x * c.S;
        const int p = st.ctr[e * fsS + lane];
        base[x * kMaxSnakes + k] = c.vr ? (p >> 8) * c.pw + (p & 255) + c.lp - c.vr : 0;
    }
}

template <int T = kWave>
__device__ __forceinline__ void zero_lean(const KCfg &c, uint8_t *pf, int lane)
{
    for (int q = lane; q < (c.fs * c.pframe) >> 4; q += T) reinterpret_cast<uint4 *>(pf)[q] = make_uint4(0, 0, 0, 0);
}

// Row-wise encode: lane = one (snake, frame, window row); the row's cells are
// scattered as single bytes into a zeroed LDS image of a group of whole snakes'
// observations, which is then copied out with 16-byte stores. Per cell: one
// frame byte read, the channel, one byte write (empty cells write nothing).
__device__ void encode_rows(const KCfg &c, const uint8_t *frames, const int *org, int slot0,
                            uint8_t *obs_env, uint8_t *stage, int lane)
{
    const int fs = c.fs, ow = c.ow, oh = c.oh, S = c.S, cellb = 8 * fs, W = c.W;
    const int P = oh * ow * cellb;
    const int fsoh = fs * oh;
    const bool wide = (c.units & 1) == 0;
    for (int k0 = 0; k0 < S; k0 += c.enc_group) {
        const int gs = min(c.enc_group, S - k0), bytes = gs * P;
        for (int q = lane; q < (bytes + 15) >> 4; q += kWave)
            reinterpret_cast<uint4 *>(stage)[q] = make_uint4(0, 0, 0, 0);
        wave_sync();
        for (int rr = lane; rr < gs * fsoh; rr += kWave) {
            const int kk = (int)__umulhi((uint32_t)rr, c.mag_fsoh), rem = rr - kk * fsoh;
            const int f = (int)__umulhi((uint32_t)rem, c.mag_oh), i = rem - f * oh;
            const int k = k0 + kk;
            int s = slot0 + f;
            s -= (s >= fs) ? fs : 0;
            const int p = org[s * kMaxSnakes + k];
            const int r = (p >> 16) - 256 + i, c0 = (p & 0xffff) - 256;
            if ((unsigned)r >= (unsigned)c.H) continue;
            const uint8_t *row = frames + s * c.grid_stride + r * W;
            uint8_t *dst = stage + kk * P + i * ow * cellb + f * 8;
            for (int j = 0; j < ow; j++) {
                const int cc = c0 + j;
                const int v = ((unsigned)cc < (unsigned)W) ? row[cc] : 0;
                const int id = div10(v), code = v - 10 * id;
                const int ch = (v < 3) ? v - 1 : code - 1 + ((id == k) ? 3 : 0);
                if (v != 0) dst[j * cellb + ch] = 1;
            }
        }
        wave_sync();
        uint8_t *out = obs_env + (int64_t)k0 * P;
        if (wide) {
            for (int q = lane; q < bytes >> 4; q += kWave)
                obs_store(reinterpret_cast<v4u *>(out) + q, reinterpret_cast<const v4u *>(stage)[q]);
        } else {
            for (int q = lane; q < bytes >> 3; q += kWave)
                obs_store(reinterpret_cast<v2u *>(out) + q, reinterpret_cast<const v2u *>(stage)[q]);
        }
        wave_sync();
    }
}

__device__ __forceinline__ void encode_obs(const KCfg &c, const uint8_t *frames, const int *org, int slot0,
                                           uint8_t *obs_env, uint8_t *lds, int lane)
{
    if (c.enc_group > 0) encode_rows(c, frames, org, slot0, obs_env, lds + c.lds_stage, lane);
    else encode(c, frames, org, slot0, obs_env, lane);
}

__device__ __forceinline__ int pack_origin(const KCfg &c, int r, int cc)
{
    return c.vr ? (((r - c.vr + 256) << 16) | (cc - c.vr + 256)) : ((256 << 16) | 256);
}

// Copy bytes [0, n) (n % 16 == 0) global -> LDS, 16 B per lane, up to four
// loads in flight per lane before the LDS writes.
__device__ __forceinline__ void stage_to_lds(uint8_t *dst, const uint8_t *src, int n, int lane)
{
    const int n16 = n >> 4;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    for (int q = lane; q < n16; q += 4 * kWave) {
        const int q1 = q + kWave, q2 = q + 2 * kWave, q3 = q + 3 * kWave;
        const uint4 a = s4[q];
        const uint4 b = q1 < n16 ? s4[q1] : a;
        const uint4 c = q2 < n16 ? s4[q2] : a;
        const uint4 d = q3 < n16 ? s4[q3] : a;
        d4[q] = a;
        if (q1 < n16) d4[q1] = b;
        if (q2 < n16) d4[q2] = c;
        if (q3 < n16) d4[q3] = d;
    }
}

// ---------------------------------------------------- step: the observation
// After k_logic, one launch (k_post / k_post_lean, launch_step): reset workers
// (the queued auto-resets, latency-bound, many registers, draw record in LDS,
// then the in-step spawn-ahead jobs) and the encodes of every other env's
// stacked frames (bandwidth-bound).
// The observation of env e's current frame stack (_get_obs, snake_env.py:461-472):
// the grid ring and crop centres staged in LDS, then the (staged) encode.
__device__ __forceinline__ void encode_env(const KCfg &c, const snake_state &st, const snake_out &o, int e,
                                           uint8_t *lds, int lane)
{
    const int fs = c.fs, S = c.S;
    uint8_t *frames = lds + c.lds_frames;
    int *org = reinterpret_cast<int *>(lds + c.lds_centers);
    const int cur = st.env[(int64_t)e * kEnvRec + ENV_CUR];
    stage_to_lds(frames, st.grid + (int64_t)e * c.ring_bytes, c.ring_bytes, lane);
    for (int q = lane; q < fs * S; q += kWave) {
        const int x = q / S, k = q - x * S;
        const int p = st.ctr[(int64_t)e * fs * S + q];
        org[x * kMaxSnakes + k] = pack_origin(c, p >> 8, p & 255);
    }
    wave_sync();
    encode_obs(c, frames, org, cur + 1 == fs ? 0 : cur + 1, o.obs + (int64_t)e * c.units * 8, lds, lane);
}

__device__ __forceinline__ void encode_one(const KCfg &c, const snake_state &st, const snake_out &o, const int e)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x;
    // a reset env's obs is written by its reset; in every-step mode only the
    // envs rejected for an invalid action (left unchanged) are not reset
    if (c.autoreset == 2 ? o.err[e] != 1 : (c.autoreset && o.ep_done[e])) return;
    encode_setprio(c);
    encode_env(c, st, o, e, lds, lane);
}

// k_encode over c.enc_per_wave consecutive envs per wave: the next env's grid
// ring, current slot, crop centres and reset flag are loaded into registers
// before this env's encode, so their memory round trip overlaps it (a
// one-env wave waits for its ring with nothing else to do; the encode is
// latency- and occupancy-bound beside the reset workers). NPF = 16-byte ring
// chunks per lane kept in flight (ring_bytes <= NPF * 1024).
template <int NPF>
__device__ __forceinline__ void encode_multi(const KCfg &c, const snake_state &st, const snake_out &o, const int b)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x;
    encode_setprio(c);
    const int fs = c.fs, S = c.S, n16 = c.ring_bytes >> 4, fsS = fs * S;
    uint8_t *frames = lds + c.lds_frames;
    int *org = reinterpret_cast<int *>(lds + c.lds_centers);
    const int e_begin = b * c.enc_per_wave, e_end = min(c.N, e_begin + c.enc_per_wave);
    // (one vector value, not an array: an array of uint4 carried across the
    // loop was demoted to scratch)
    typedef uint32_t pf_t __attribute__((ext_vector_type(4 * NPF)));
    pf_t pf = {};
    int pcur = 0, pctr = 0, pskip = 0;
    // (this prefetch and the table and lean encodes' are macros, not lambdas: as
    // lambdas every k_post and k_post_lean instantiation compiled to other code)
#define SNAKE_ENC_FETCH(EE)                                                                       \
    do {                                                                                           \
        const int64_t e_ = (EE);                                                                   \
        const uint4 *src_ = reinterpret_cast<const uint4 *>(st.grid + e_ * c.ring_bytes);          \
        _Pragma("unroll") for (int u = 0; u < NPF; u++) {   /* (clamped: no per-chunk branch) */   \
            const uint4 x_ = src_[min(lane + u * kWave, n16 - 1)];                                 \
            pf[4 * u] = x_.x; pf[4 * u + 1] = x_.y; pf[4 * u + 2] = x_.z; pf[4 * u + 3] = x_.w;     \
        }                                                                                          \
        pcur = st.env[e_ * kEnvRec + ENV_CUR];                                                     \
        pctr = lane < fsS ? st.ctr[e_ * fsS + lane] : 0;                                           \
        pskip = c.autoreset ? o.ep_done[e_] : 0;                                                   \
    } while (0)
    if (e_begin < e_end) SNAKE_ENC_FETCH(e_begin);
    for (int e = e_begin; e < e_end; e++) {
        const int cur = pcur, skip = pskip;   // (its reset writes the obs of a reset env)
        if (!skip) {
            uint4 *d4 = reinterpret_cast<uint4 *>(frames);
#pragma unroll
            for (int u = 0; u < NPF; u++)
                d4[min(lane + u * kWave, n16 - 1)] = make_uint4(pf[4 * u], pf[4 * u + 1], pf[4 * u + 2], pf[4 * u + 3]);
            if (lane < fsS) {
                const int x = lane / S, k = lane - x * S;
                org[x * kMaxSnakes + k] = pack_origin(c, pctr >> 8, pctr & 255);
            }
        }
        if (e + 1 < e_end) SNAKE_ENC_FETCH(e + 1);   // in flight during this env's encode
        if (!skip) {
            wave_sync();
            encode_obs(c, frames, org, cur + 1 == fs ? 0 : cur + 1, o.obs + (int64_t)e * c.units * 8, lds, lane);
            wave_sync();   // the LDS frames are rewritten for the next env
        }
    }
#undef SNAKE_ENC_FETCH
}

// ---------------------------------------------------------- table encode
// The observation of c.enc_per_wave consecutive envs per wave (_encode
// snake_env.py:474-519 + the frame stack :444-472) as table lookups. Per 8-byte
// unit (snake k, window row i, column j, frame f: obs (S, oh, ow, 8 fs)) the grid
// byte v of frame f at that window cell comes from a zero-bordered LDS image of
// the env's frames (no bounds test: cells outside the grid read 0), and the
// unit's 8 one-hot channels are the table entry pat[k][v] (onehot(); v < 10 * S,
// so c.tbl_patv = 10 * S entries per snake). A lane's units are the same for
// every env: their descriptors desc[u] = (i * pw + j) | (f * 16 + k) << 16 are
// built once per wave -- straight into registers where a lane's chunks take
// one pass, else into an LDS table -- and per env only the window origins
// base[f * 16 + k] = (LDS byte of the window origin in frame f, byte offset of
// pat[k]) change. Per 16-byte store: one descriptor pair, two window origins,
// two grid bytes and two patterns from LDS, four address adds. The next env's
// frames (NPW dwords per lane), slot, crop centres and reset flag are loaded
// into registers during this env's encode (as encode_lean_block); the first
// env's before the wave's setup, so that round trip runs beside it. The
// setup's divisions are multiply-highs by plan-time reciprocals (mag_*).
template <int T>
__device__ __forceinline__ void tsync()
{
    if constexpr (T == kWave) wave_sync();
    else __syncthreads();
}

// FU (k_step): the frames and the hand-off record (slot, reset flag, crop
// centres) of the logic wave that finished these envs in this launch, all read
// with write-through-coherent (sc1) loads after its done flag.
// One-wave form (T = kWave): `wave` = this wave's index in its workgroup
// (k_post runs c.enc_wpb independent encode waves per workgroup, each on its
// own c.lds_tbl_bytes of LDS and synchronising at wave level only).
template <int NPW, int T, bool FU>
__device__ __forceinline__ void encode_tbl_body(const KCfg &c, const snake_state &st, const snake_out &o, const int blk,
                                                const int wave)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds0[];
    uint8_t *lds = lds0 + wave * c.lds_tbl_bytes;
    const int lane = threadIdx.x & (T - 1);
    encode_setprio(c);
    uint8_t *pf = lds;                                                   // fs * pframe bytes
    uint2 *base = reinterpret_cast<uint2 *>(lds + c.tbl_base);           // [fs][16]
    uint8_t *pat = lds + c.tbl_pat;                                      // uint2 [S][c.tbl_patv]
    uint32_t *desc = reinterpret_cast<uint32_t *>(lds + c.tbl_desc);     // [units] (carved for the multi-pass forms only)
    const int S = c.S, fs = c.fs, fsS = fs * S;
    const int wpr = c.W >> 2, nw = c.H * wpr, nwt = fs * nw, gsw = c.grid_stride >> 2;
    // per prefetched dword: ring word index and LDS dword index (clamped: the
    // lanes past the end repeat the last word, same source, same destination)
    int src[NPW], dst[NPW];
#pragma unroll
    for (int u = 0; u < NPW; u++) {
        const int x = min(lane + u * T, nwt - 1);
        const int s = fdiv((uint32_t)x, c.mag_nw, nw), xx = x - s * nw;
        const int r = fdiv((uint32_t)xx, c.mag_wpr, wpr), c4 = xx - r * wpr;
        src[u] = s * gsw + xx;
        dst[u] = (s * c.pframe + (r + c.vr) * c.pw + c.lp) / 4 + c4;
    }
    const int e_begin = blk * c.enc_per_wave, e_end = min(c.N, e_begin + c.enc_per_wave);
    uint32_t w[NPW];
    int pcur = 0, pctr = 0, pskip = 0;
#define SNAKE_TBL_FETCH(EE)                                                                  \
    do {                                                                                           \
        const int64_t e_ = (EE);                                                                   \
        const uint32_t *r32_ = reinterpret_cast<const uint32_t *>(st.grid + e_ * c.ring_bytes);    \
        if constexpr (FU) {                                                                        \
            _Pragma("unroll") for (int u = 0; u < NPW; u++) w[u] = ld_sc1(r32_ + src[u]);          \
            const uint4 h_ = ld_sc1_128(st.resetq + c.fu_hoff + 4 * e_);                           \
            pcur = (int)(h_.x & 255u);                                                             \
            pskip = (int)((h_.x >> 8) & 1u);                                                       \
            pctr = lane < fsS ? (int)(((lane < 2 ? h_.y : h_.z) >> (16 * (lane & 1))) & 0xffffu) : 0; \
        } else {                                                                                   \
            _Pragma("unroll") for (int u = 0; u < NPW; u++) w[u] = r32_[src[u]];                   \
            pcur = st.env[e_ * kEnvRec + ENV_CUR];                                                 \
            pctr = lane < fsS ? st.ctr[e_ * fsS + lane] : 0;                                       \
            pskip = c.autoreset ? o.ep_done[e_] : 0;                                               \
        }                                                                                          \
    } while (0)
    // the first env's frames, slot, centres and reset flag: issued before the
    // setup below, so their memory round trip runs beside it
    if (e_begin < e_end) SNAKE_TBL_FETCH(e_begin);
    // once per wave: the zero image, the patterns of the codes that occur (0, 1,
    // 2 and 10 * id + 3..5 for id < S; c.tbl_patv entries per snake), the unit
    // descriptors
    zero_lean<T>(c, pf, lane);
    const int npv = 3 + 3 * S, patv = c.tbl_patv;   // occurring codes per snake, table entries per snake
    for (int x = lane; x < S * npv; x += T) {
        const int k = (int)__umulhi((uint32_t)x, c.mag_npv), r = x - k * npv;
        const int v = r < 3 ? r : 10 * ((r - 3) / 3) + 3 + (r - 3) % 3;
        const unsigned long long b = onehot(v, k);
        reinterpret_cast<uint2 *>(pat)[k * patv + v] = make_uint2((uint32_t)b, (uint32_t)(b >> 32));
    }
    auto desc_of = [&](const int u) {
        const int kk = (int)__umulhi((uint32_t)u, c.mag_ups), r0 = u - kk * c.ups;
        const int ii = (int)__umulhi((uint32_t)r0, c.mag_rowl), r1 = r0 - ii * c.rowl;
        const int jj = fdiv((uint32_t)r1, c.mag_fs, fs), ff = r1 - jj * fs;
        return (uint32_t)(ii * c.pw + jj) | ((uint32_t)(ff * kMaxSnakes + kk) << 16);
    };
    const int chunks = c.units >> 1;
    // a lane's chunks all in one pass (cfg3: 242 chunks): their descriptors
    // computed straight into registers for every env of the wave -- no LDS
    // table (not carved: tbl_desc_in_lds), one LDS level less per lookup chain
    const bool one = T == kWave && chunks <= 4 * T;
    uint2 dr[4];
    if constexpr (T == kWave) if (one) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int q = min(t * T + lane, chunks - 1);
            dr[t] = make_uint2(desc_of(2 * q), desc_of(2 * q + 1));
        }
    }
    if (!one)
        for (int u = lane; u < c.units; u += T) desc[u] = desc_of(u);
    for (int e = e_begin; e < e_end; e++) {
        const int cur = pcur, skip = pskip;   // (a reset env's obs is written by its reset)
        tsync<T>();                          // (the previous encode has read the LDS image)
        if (!skip) {
#pragma unroll
            for (int u = 0; u < NPW; u++) reinterpret_cast<uint32_t *>(pf)[dst[u]] = w[u];
            if (lane < fsS) {
                // ring slot s = lane / S holds frame f = s - (the oldest slot), mod fs
                const int s = fdiv((uint32_t)lane, c.mag_S, S), k = lane - s * S, slot0 = cur + 1 == fs ? 0 : cur + 1;
                const int f = s >= slot0 ? s - slot0 : s - slot0 + fs;
                const uint32_t gb = (uint32_t)(s * c.pframe) +
                                    (c.vr ? (uint32_t)((pctr >> 8) * c.pw + (pctr & 255) + c.lp - c.vr) : 0u);
                base[f * kMaxSnakes + k] = make_uint2(gb, (uint32_t)(k * patv * 8));
            }
        }
        if (e + 1 < e_end) SNAKE_TBL_FETCH(e + 1);   // in flight during this env's encode
        if (!skip) {
            tsync<T>();
            const auto rs = __builtin_amdgcn_make_buffer_rsrc(o.obs + (int64_t)e * c.units * 8, 0, c.units * 8, 0x00020000);
            auto lookup = [&](uint2 dd) {   // units 2q, 2q + 1 of descriptor pair dd
                const uint2 b0 = base[dd.x >> 16], b1 = base[dd.y >> 16];
                const uint32_t v0 = pf[b0.x + (dd.x & 0xffffu)], v1 = pf[b1.x + (dd.y & 0xffffu)];
                const uint2 p0 = *reinterpret_cast<const uint2 *>(pat + b0.y + 8 * v0);
                const uint2 p1 = *reinterpret_cast<const uint2 *>(pat + b1.y + 8 * v1);
                return (v4u){p0.x, p0.y, p1.x, p1.y};
            };
            if (T == kWave && one) {
                v4u r[4];
#pragma unroll
                for (int t = 0; t < 4; t++) r[t] = lookup(dr[t]);
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (t * T + lane < chunks) obs_store_rs(rs, 16 * (t * T + lane), r[t]);
            } else {
            // CP chunks per lane and pass, their lookup chains interleaved
            // (clamped reads; only the chunks that exist are stored); two in
            // four-wave workgroups (register budget)
            constexpr int CP = T == kWave ? 4 : 2;
            for (int q0 = 0; q0 < chunks; q0 += CP * T) {
                v4u r[CP];
#pragma unroll
                for (int t = 0; t < CP; t++)
                    r[t] = lookup(reinterpret_cast<const uint2 *>(desc)[min(q0 + t * T + lane, chunks - 1)]);
#pragma unroll
                for (int t = 0; t < CP; t++)
                    if (q0 + t * T + lane < chunks) obs_store_rs(rs, 16 * (q0 + t * T + lane), r[t]);
            }
            }
        }
    }
#undef SNAKE_TBL_FETCH
}

// Inlined into its kernels, except the one-wave form with eight frame dwords
// per lane (larger boards, 16 kernels): that one stays a function, as the
// inliner had left it. Pinned here because the setup's size decides the
// inliner's choice otherwise, and an out-of-line two-dword form costs k_post
// 118 VGPRs instead of 71.
template <bool FU>
__device__ __noinline__ void encode_tbl_block8(const KCfg &c, const snake_state &st, const snake_out &o, const int blk,
                                               const int wave)
{
    encode_tbl_body<8, kWave, FU>(c, st, o, blk, wave);
}

template <int NPW, int T = kWave, bool FU = false>
__device__ __forceinline__ void encode_tbl_block(const KCfg &c, const snake_state &st, const snake_out &o, const int blk,
                                                 const int wave = 0)
{
    if constexpr (NPW == 8 && T == kWave) encode_tbl_block8<FU>(c, st, o, blk, wave);
    else encode_tbl_body<NPW, T, FU>(c, st, o, blk, wave);
}

// Lean encode over c.enc_per_wave consecutive envs per workgroup of T = 256
// threads (W % 4 == 0, rings of 513 to 2 048 dwords: cfg5's 40x40 x 4 frames):
// the next env's frames (NPW dwords per thread), current slot, crop centres and
// reset flag are loaded into registers while this env is encoded, one memory
// round trip per env in the shadow of the previous encode; the zero border of
// the LDS image is written once per workgroup. The LDS destination of every
// prefetched dword is the same for every env (computed once). Four waves share
// one LDS image (cfg5 k_encode 91 -> 66 us against one wave per env, round 3).
template <int NPW, int T>
__device__ __forceinline__ void encode_lean_block(const KCfg &c, const snake_state &st, const snake_out &o,
                                                  const int blk)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x;
    encode_setprio(c);
    uint8_t *pf = lds;
    int *base = reinterpret_cast<int *>(lds + c.fs * c.pframe);
    uint32_t *p32 = reinterpret_cast<uint32_t *>(pf);
    const int wpr = c.W >> 2, nw = c.H * wpr, nwt = c.fs * nw, gsw = c.grid_stride >> 2, fsS = c.fs * c.S;
    // per prefetched dword: ring word index and LDS dword index (clamped: the
    // threads past the end repeat the last word, same source, same destination)
    int src[NPW], dst[NPW];
#pragma unroll
    for (int u = 0; u < NPW; u++) {
        const int x = min(lane + u * T, nwt - 1);
        const int s = x / nw, xx = x - s * nw;
        const int r = fdiv((uint32_t)xx, c.mag_wpr, wpr), c4 = xx - r * wpr;
        src[u] = s * gsw + xx;
        dst[u] = (s * c.pframe + (r + c.vr) * c.pw + c.lp) / 4 + c4;
    }
    zero_lean<T>(c, pf, lane);
    const int e_begin = blk * c.enc_per_wave, e_end = min(c.N, e_begin + c.enc_per_wave);
    uint32_t w[NPW];
    int pcur = 0, pctr = 0, pskip = 0;
#define SNAKE_LEAN_FETCH(EE)                                                                       \
    do {                                                                                           \
        const int64_t e_ = (EE);                                                                   \
        const uint32_t *r32_ = reinterpret_cast<const uint32_t *>(st.grid + e_ * c.ring_bytes);    \
        _Pragma("unroll") for (int u = 0; u < NPW; u++) w[u] = r32_[src[u]];                       \
        pcur = st.env[e_ * kEnvRec + ENV_CUR];                                                     \
        pctr = lane < fsS ? st.ctr[e_ * fsS + lane] : 0;                                           \
        pskip = c.autoreset ? o.ep_done[e_] : 0;                                                   \
    } while (0)
    if (e_begin < e_end) SNAKE_LEAN_FETCH(e_begin);
    for (int e = e_begin; e < e_end; e++) {
        const int cur = pcur, skip = pskip;   // (a reset env's obs is written by its reset)
        tsync<T>();                           // (the previous encode has read the LDS image)
        if (!skip) {
#pragma unroll
            for (int u = 0; u < NPW; u++) p32[dst[u]] = w[u];
            if (lane < fsS) {
                const int x = lane / c.S, k = lane - x * c.S;
                base[x * kMaxSnakes + k] = c.vr ? (pctr >> 8) * c.pw + (pctr & 255) + c.lp - c.vr : 0;
            }
        }
        if (e + 1 < e_end) SNAKE_LEAN_FETCH(e + 1);   // in flight during this env's encode
        if (!skip) {
            tsync<T>();
            encode_lean<T>(c, pf, base, cur + 1 == c.fs ? 0 : cur + 1, o.obs + (int64_t)e * c.units * 8, lane);
        }
    }
#undef SNAKE_LEAN_FETCH
}

}  // namespace snake
