// snake_launch.inc -- the host layer, included at the end of snake_kernels.hip
// (one translation unit): kernel timing, the background-stream context, the
// launchers, snake_timing_* and snake_debug_set.
namespace snake {

// Every launch goes through hipExtLaunchKernel: while a launch is timed
// (TimedLaunch, snake_timing_enable) these are its start/stop events, which then
// carry the dispatch's own begin/end timestamps -- no marker packets of their
// own between the step's kernels (hipEventRecord pairs left 6 + 10.5 us gaps
// around each timed step's k_logic / k_post in the kernel trace). Null: a
// plain launch.
thread_local hipEvent_t t_ev0 = nullptr, t_ev1 = nullptr;
template <typename F, typename... Args>
static inline void slaunch(F kernel, const dim3 &grid, const dim3 &block, uint32_t lds, hipStream_t s,
                           Args... args)
{
    hipExtLaunchKernelGGL(kernel, grid, block, lds, s, t_ev0, t_ev1, 0u, args...);
}

// ------------------------------------------------------------- kernel timing
// Profiling aid (snake_timing_enable / snake_timing_read): pairs of timing events
// around each launch, resolved when read. Event objects are pooled.
namespace {
struct TimingRec {
    const char *name;
    hipEvent_t a, b;
};
std::mutex g_tmu;
bool g_timing = false;
int g_draw_wait_ticks = 200000;   // KCfg.draw_wait (snake_debug_set "draw_wait_ticks")
int g_spawn_delay_ticks = 0;      // KCfg.spawn_delay (snake_debug_set "spawn_delay_ticks")
int g_fuse_roles = 7;             // KCfg.fu_roles (snake_debug_set "fuse_roles", diagnostics)
#ifndef SNAKE_FUSED
#define SNAKE_FUSED 0
#endif
int g_fused = SNAKE_FUSED;        // the fused step where KCfg.fused allows it (snake_debug_set "fused")
std::vector<TimingRec> g_pending;
std::vector<hipEvent_t> g_pool;
std::map<std::string, std::pair<double, int64_t>> g_done;

hipEvent_t pooled_event()
{
    if (!g_pool.empty()) {
        hipEvent_t ev = g_pool.back();
        g_pool.pop_back();
        return ev;
    }
    hipEvent_t ev = nullptr;
    // timing only: no system-scope fence (cache write-back and invalidate) when
    // the event completes, which would delay the next kernel
    if (hipEventCreateWithFlags(&ev, hipEventDisableSystemFence) != hipSuccess) return nullptr;
    return ev;
}
}  // namespace

// Times the one launch (slaunch) made between its construction and close():
// the pair of pooled events rides on that launch (no-ops when timing is off).
struct TimedLaunch {
    const char *name;
    hipEvent_t a = nullptr, b = nullptr;
    TimedLaunch(const char *n, hipStream_t) : name(n)
    {
        std::lock_guard<std::mutex> g(g_tmu);
        if (!g_timing) return;
        a = pooled_event();
        b = a ? pooled_event() : nullptr;
        if (!b) {
            if (a) g_pool.push_back(a);
            a = nullptr;
            return;
        }
        t_ev0 = a;
        t_ev1 = b;
    }
    void close()
    {
        if (!a) return;
        t_ev0 = t_ev1 = nullptr;
        std::lock_guard<std::mutex> g(g_tmu);
        // (a failed launch records neither: launch_status reports it, the pair
        // goes back to the pool)
        if (hipPeekAtLastError() == hipSuccess) g_pending.push_back({name, a, b});
        else {
            g_pool.push_back(a);
            g_pool.push_back(b);
        }
        a = nullptr;
    }
    ~TimedLaunch() { close(); }
};

// ---------------------------------------------------------------- launchers
// (each under a DeviceGuard and checked by launch_status, snake_device.h)

// The background stream's events only order kernels of one device: no
// system-scope fence (that would write the L2s back for a host that never looks).
constexpr unsigned kJoinFlags = hipEventDisableTiming | hipEventDisableSystemFence;

// Background spawn-ahead (KCfg.bg) per state (keyed by its env records): the
// stream k_spawn runs on, the event the caller's stream records after k_logic
// (k_spawn's start), the event recorded after the last k_spawn of each queue
// set, the step counter whose parity picks the queue set. Created by the
// state's first step, destroyed by snake_release.
// One background stream per queue set (round 5): a set's k_spawn only waits for
// that set's previous one, so consecutive steps' spawn kernels may overlap --
// with one stream they queued behind each other (a 40x40 job takes about a
// step) and k_logic found its set's previous kernel unfinished in ~21 % of
// cfg5's steps, queued nothing, and the next step's resets drew inline.
constexpr int kBgStreams = 2;
struct BgCtx {
    // (two streams for the four queue sets, set p on stream p % 2: every
    // stream takes one of the process's hardware queues -- GPU_MAX_HW_QUEUES,
    // 4 by default -- and with four background streams the caller's stream
    // shared one with a spawn kernel: cfg5 0.0811 -> 0.0980 ms, round 6)
    hipStream_t x[kBgStreams] = {};
    hipEvent_t fork = nullptr;
    hipEvent_t done[kQSets] = {};
    uint64_t steps = 0;
    bool pending[kQSets] = {};
    uint32_t launched[kQSets] = {};   // k_spawn launches per queue set (KCfg.spawn_gate)
};
static std::mutex g_bgmu;
static std::map<const void *, BgCtx> g_bg;
// The fused step's per-state epoch (k_step): the number of k_step launches of
// the state so far; its flag area is zeroed on the state's first fused step.
static std::map<const void *, uint32_t> g_fu;

static void destroy_bg(BgCtx &c)
{
    for (hipStream_t x : c.x)
        if (x) (void)hipStreamSynchronize(x);   // (its last k_spawn)
    if (c.fork) (void)hipEventDestroy(c.fork);
    for (hipEvent_t ev : c.done)
        if (ev) (void)hipEventDestroy(ev);
    for (hipStream_t x : c.x)
        if (x) (void)hipStreamDestroy(x);
    c = BgCtx();
}

static BgCtx *bg_ctx(const snake_state &st, bool create)
{
    std::lock_guard<std::mutex> g(g_bgmu);
    auto it = g_bg.find(st.env);
    if (it != g_bg.end()) return &it->second;
    if (!create) return nullptr;
    BgCtx c;
    bool ok = true;
    for (int p = 0; p < kBgStreams && ok; p++)
        ok = hipStreamCreateWithFlags(&c.x[p], hipStreamNonBlocking) == hipSuccess;
    for (int p = 0; p < kQSets && ok; p++)
        ok = hipEventCreateWithFlags(&c.done[p], kJoinFlags) == hipSuccess;
    // (the fork event rides on k_logic's dispatch as its stop event, like the
    // timing events: a timing-capable event without the system fence)
    if (!ok || hipEventCreateWithFlags(&c.fork, hipEventDisableSystemFence) != hipSuccess) {
        destroy_bg(c);
        set_error("background stream / event creation failed");
        return nullptr;
    }
    return &g_bg.emplace(st.env, c).first->second;   // (std::map: the address stays valid)
}

// `stream` waits for the state's last background spawn kernel (if any).
int wait_background(const snake_state &st, void *stream)
{
    BgCtx *b = bg_ctx(st, false);
    if (!b) return SNAKE_OK;
    for (int p = 0; p < kQSets; p++)
        if (b->pending[p] && hipStreamWaitEvent((hipStream_t)stream, b->done[p], 0) != hipSuccess) {
            set_error("waiting for the background spawn kernel failed");
            return SNAKE_E_LAUNCH;
        }
    return SNAKE_OK;
}

// The state's background context (snake_release): its last spawn kernel
// waited for on the host, its stream and events destroyed, the entry erased,
// so an allocation that later reuses the same env address starts afresh.
int release_background(const snake_state &st)
{
    BgCtx c;
    {
        std::lock_guard<std::mutex> g(g_bgmu);
        g_fu.erase(st.env);
        auto it = g_bg.find(st.env);
        if (it == g_bg.end()) return SNAKE_OK;
        c = it->second;
        g_bg.erase(it);
    }
    DeviceGuard dg(c.x[0]);   // (the streams' device current while they are destroyed)
    destroy_bg(c);
    return dg.dev < 0 ? SNAKE_E_LAUNCH : SNAKE_OK;
}

int launch_seed(const KCfg &k, const snake_state &st, uint32_t base_seed, int64_t env_offset, void *stream)
{
    const int threads = 256, blocks = (k.N + threads - 1) / threads;
    DeviceGuard dg((hipStream_t)stream);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    if (int rc = wait_background(st, stream)) return rc;
    slaunch(k_seed, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, k, st, base_seed, (long long)env_offset);
    return launch_status("k_seed");
}

int launch_render(const KCfg &k, const snake_state &st, const uint8_t *palette, uint8_t *rgb, void *stream)
{
    RenderPal pal;
    memcpy(pal.rgb, palette, sizeof(pal.rgb));
    DeviceGuard dg((hipStream_t)stream);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    const long long quads = ((long long)k.N * k.HW + 3) / 4;
    const int threads = 256;
    const long long blocks = (quads + threads - 1) / threads;
    slaunch(k_render, dim3((unsigned)blocks), dim3(threads), 0, (hipStream_t)stream, k, st, pal, rgb);
    return launch_status("k_render");
}

// pick<V...>(v, f): f(Int<X>{}) for the X of V... that equals v -- the last of the list when none
// does -- so a run-time value becomes a template argument (PICKED). The lists of the launchers
// below are the whole set of kernel instantiations.
template <int V> using Int = std::integral_constant<int, V>;
template <int... V, typename F>
static inline void pick(int v, F &&f)
{
    constexpr int list[] = {V...}, last = list[sizeof...(V) - 1];
    if (!((V != last && v == V ? (f(Int<V>{}), true) : false) || ...)) f(Int<last>{});
}
#define PICKED(x) decltype(x)::value

int launch_reset(const KCfg &k, const snake_state &st, const uint8_t *mask, const snake_out &o, void *stream)
{
    const dim3 grid(k.link_in_lds ? k.N : k.reset_slots), block(kWave);
    DeviceGuard dg((hipStream_t)stream);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    if (int rc = wait_background(st, stream)) return rc;
    TimedLaunch tl("k_reset", (hipStream_t)stream);
    const KArgs a{k, st, o, mask};
    const hipStream_t s = (hipStream_t)stream;
    pick<0, 1, 2>(link_record(k), [&](auto jl) {
        pick<4, 8, 16>(lanes_per_env(k.S), [&](auto ms) {
            slaunch((k_reset<PICKED(ms), PICKED(jl)>), grid, block, k.lds_bytes, s, a);
        });
    });
    tl.close();
    return launch_status("k_reset");
}

// The launch shape of the step's shared phase. k_post: the workers, then the encodes; npf (its NPF)
// = 16-byte ring chunks per lane the two-env encode keeps in flight, 0 = one env per block, -NPW =
// the table encode. k_post_lean: four workers per workgroup, then the four-wave encodes; no npf.
struct PostShape {
    int npf;
    dim3 grid, block;
    int lds;
};

static PostShape post_shape(const KCfg &k)
{
    const int epw = k.enc_per_wave;
    if (k.lean)
        return {0, dim3((k.reset_slots + 3) / 4 + (k.N + epw - 1) / epw), dim3(256),
                std::max(4 * k.lds_worker, k.tbl ? k.lds_tbl_bytes : k.lds_lean_bytes)};
    const int n16 = k.ring_bytes >> 4;
    const int npf = k.tbl ? -tbl_npw(k) : (epw <= 1 ? 0 : (n16 <= kWave ? 1 : (n16 <= 2 * kWave ? 2 : 8)));
    const int enc_waves = npf == 0 ? k.N : (k.N + epw - 1) / epw;
    // the table encode: enc_wpb independent waves per workgroup, each with its own carve
    const int wpb = k.tbl ? k.enc_wpb : 1;
    return {npf, dim3(k.reset_slots + (enc_waves + wpb - 1) / wpb), dim3(kWave * wpb),
            std::max(k.lds_bytes, k.tbl ? wpb * k.lds_tbl_bytes : k.lds_obs_bytes)};
}

// k_post_lean<MS(S), RO(bg), TBL> or k_post<MS(S), NPF, RO, JL>: resets only (ro: background
// boards, whose link_record is 1) or the workers' whole job list with the link table jl
static void launch_post(const KArgs &a, const PostShape &p, bool ro, int jl, hipStream_t s)
{
    if (a.c.lean)
        return pick<0, 1>(a.c.tbl ? 1 : 0, [&](auto tbl) {
            pick<0, 1>(a.c.bg ? 1 : 0, [&](auto bg) {
                pick<4, 8, 16>(lanes_per_env(a.c.S), [&](auto ms) {
                    slaunch((k_post_lean<PICKED(ms), PICKED(bg) != 0, PICKED(tbl) != 0>), p.grid, p.block, p.lds, s, a);
                });
            });
        });
    auto go = [&](auto ro_c, auto jl_c) {
        pick<4, 8, 16>(lanes_per_env(a.c.S), [&](auto ms) {
            pick<0, 1, 2, -2, -8, 8>(p.npf, [&](auto npf) {
                slaunch((k_post<PICKED(ms), PICKED(npf), PICKED(ro_c) != 0, PICKED(jl_c)>), p.grid, p.block, p.lds, s, a);
            });
        });
    };
    if (ro) go(Int<1>{}, Int<1>{});
    else pick<0, 1, 2>(jl, [&](auto jl_c) { go(Int<0>{}, jl_c); });
}

static int launch_encode(const KCfg &k, const snake_state &st, const snake_out &o, hipStream_t sm)
{
    TimedLaunch t3("k_encode", sm);
    slaunch(k_encode, dim3(k.N), dim3(kWave), k.lds_obs_bytes, sm, k, st, o);
    t3.close();
    return launch_status("k_encode");
}

// The whole step as one launch (k_step), on the state's next epoch.
static int launch_fused(KCfg &k, const snake_state &st, const int8_t *actions, const snake_out &o, hipStream_t sm)
{
    uint32_t ep;
    bool fresh = false;
    {
        std::lock_guard<std::mutex> g(g_bgmu);
        auto it = g_fu.find(st.env);
        if (it == g_fu.end()) { it = g_fu.emplace(st.env, 0u).first; fresh = true; }
        ep = it->second;
    }
    if (fresh && hipMemsetAsync(st.resetq + k.fu_ldone, 0, sizeof(int) * (fused_area(k.N).end - k.fu_ldone), sm) != hipSuccess) {
        set_error("zeroing the fused step's flags failed");
        return SNAKE_E_LAUNCH;
    }
    k.epoch = ep + 1;
    const dim3 gf(k.nlg + k.reset_slots + (k.N + 3) / 4), bf(kWave);
    const int lds_f = std::max(k.lds_logic, std::max(k.lds_bytes, k.lds_tbl_bytes));
    const KArgs fa{k, st, o, actions};
    TimedLaunch tf("k_step", sm);
    pick<4, 8>(k.logic_ms, [&](auto ms) {
        pick<2, 8>(tbl_npw(k), [&](auto npw_c) {
            pick<2, 1>(link_record(k), [&](auto jl) {
                slaunch((k_step<PICKED(ms), PICKED(npw_c), PICKED(jl)>), gf, bf, lds_f, sm, fa);
            });
        });
    });
    tf.close();
    if (int rc = launch_status("k_step")) return rc;
    std::lock_guard<std::mutex> g(g_bgmu);
    g_fu[st.env] = ep + 1;
    return SNAKE_OK;
}

// k_logic. Background spawn-ahead: the fork onto the background stream
// (fork_ev) is k_logic's own dispatch -- its stop event (the timing event when
// the launch is timed) -- not an event record of its own on the caller's
// stream: that marker packet stood between k_logic and k_post, 5.3 us of idle
// GPU per step at 8 192 envs (round 6 kernel trace).
static int launch_logic(const KCfg &k, const snake_state &st, const int8_t *actions, const snake_out &o,
                        BgCtx *bgc, hipEvent_t &fork_ev, hipStream_t sm)
{
    TimedLaunch t1("k_logic", sm);
    if (bgc) {
        if (!t_ev1) t_ev1 = bgc->fork;
        fork_ev = t_ev1;
    }
    const KArgs la{k, st, o, actions};
    const unsigned epw = kWave / k.logic_ms, groups = (k.N + epw - 1) / epw;   // envs per k_logic wave, waves
    // four waves (groups) per workgroup where their LDS fits (KCfg.logic_wpb):
    // k_logic cfg4 20.4 -> 19.4 us, cfg5 21.9 -> 21.1 against one (round 4)
    pick<4, 1>(k.logic_wpb, [&](auto wpb) {
        constexpr int WPB = PICKED(wpb);
        const dim3 glb((groups + WPB - 1) / WPB), blb(kWave * WPB);
        pick<0, 1>(k.bg ? 1 : 0, [&](auto bg) {
            pick<4, 8, 16>(k.logic_ms, [&](auto ms) {
                slaunch((k_logic<PICKED(ms), WPB, PICKED(bg) != 0>), glb, blb, WPB * k.lds_logic, sm, la);
            });
        });
    });
    if (bgc && fork_ev == bgc->fork) t_ev1 = nullptr;
    t1.close();
    return launch_status("k_logic");
}

// After k_logic has filled this step's queue set, a failure zeroes its
// counters, so the next step does not run this step's queues. Once k_spawn is
// launched it owns the set's spawn counters (it reads them and re-zeroes them
// at its end, ADVICE r4): only the reset counters are zeroed then -- queue 0's
// shard counts and the claim / done counters. Returns r.
static int step_fail(const KCfg &k, const snake_state &st, BgCtx *bgc, bool spawn_launched, hipStream_t sm, int r)
{
    int *qc = st.resetq + (int64_t)k.qpar * (kNumQ * kQShards * k.q_cap + kQCounters) + kNumQ * kQShards * k.q_cap;
    if (!spawn_launched) {
        // (ordered after the set's previous k_spawn, which may still use its
        // spawn and claim counters on its background stream)
        if (bgc && bgc->pending[k.qpar]) (void)hipStreamWaitEvent(sm, bgc->done[k.qpar], 0);
        (void)hipMemsetAsync(qc, 0, sizeof(int) * kQSpGen * kQSpread, sm);   // (not the finished count)
    } else {
        (void)hipMemsetAsync(qc, 0, sizeof(int) * kQShards * kQSpread, sm);
        (void)hipMemsetAsync(qc + kQClaim * kQSpread, 0, sizeof(int) * (kQDone + 1 - kQClaim) * kQSpread, sm);
    }
    return r;
}

// This step's spawn kernel on the background stream once k_logic has passed
// (fork_ev); not joined (k_logic two steps later only queues into the set once
// it has finished). A failure has gone through step_fail.
static int launch_spawn(const KCfg &k, const snake_state &st, const snake_out &o, BgCtx *bgc, hipEvent_t fork_ev, hipStream_t sm)
{
    hipStream_t bx = bgc->x[k.qpar % kBgStreams];
    if (hipStreamWaitEvent(bx, fork_ev, 0) != hipSuccess) {
        set_error("fork to the background stream failed");
        return step_fail(k, st, bgc, false, sm, SNAKE_E_LAUNCH);
    }
    KCfg ks = k;
    ks.lds_link = 0;   // (only the draw record)
    const int lds_sp = (int)draw_record_bytes(k.n_cand);
    TimedLaunch t4("k_spawn", bx);
    const KArgs sa{ks, st, o, nullptr};
    pick<4, 8, 16>(lanes_per_env(k.S), [&](auto ms) {
        slaunch(k_spawn<PICKED(ms)>, dim3(k.spawn_slots), dim3(kWave), lds_sp, bx, sa);
    });
    t4.close();
    if (int rc = launch_status("k_spawn")) return step_fail(k, st, bgc, false, sm, rc);
    // (counted as soon as it is launched: its last worker adds one to the
    // set's finished count whatever fails after this point)
    bgc->launched[k.qpar]++;
    bgc->steps++;
    if (hipEventRecord(bgc->done[k.qpar], bx) != hipSuccess) {
        // (pending / done[] would not cover this k_spawn, which writes
        // records, env word 4 and the set's counters: wait for it here so
        // that snake_sync and the next steps need not)
        (void)hipStreamSynchronize(bx);
        set_error("background spawn event failed");
        return step_fail(k, st, bgc, true, sm, SNAKE_E_LAUNCH);
    }
    bgc->pending[k.qpar] = true;
    return SNAKE_OK;
}

// snake_step: k_logic, then (all-done auto-reset) the shared phase as ONE launch
// on the caller's stream -- k_post, or k_post_lean on boards with four-wave lean
// encodes -- with, on background spawn-ahead boards, k_spawn forked onto the
// state's background stream after k_logic and not joined.
int launch_step(const KCfg &k0, const snake_state &st, const int8_t *actions, const snake_out &o, void *stream)
{
    KCfg k = k0;   // the per-step patch: the knobs, then (below) the queue set
    k.diag = g_timing ? 1 : 0;
    k.draw_wait = g_draw_wait_ticks;
    k.spawn_delay = g_spawn_delay_ticks;
    k.fu_roles = g_fuse_roles;
    const hipStream_t sm = (hipStream_t)stream;
    DeviceGuard dg(sm);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    // everything that can fail before k_logic fills this step's queue set
    BgCtx *bgc = nullptr;
    if (k.bg) {   // background spawn-ahead: this step's queue set; k_logic queues
                  // spawn-ahead jobs into it only if the spawn kernels launched on
                  // it so far have finished (kQSpGen), the stream never waits
                  // (the wait cost cfg5 0.1026 -> 0.1136 ms per step)
        if (!(bgc = bg_ctx(st, true))) return SNAKE_E_LAUNCH;
        k.qpar = (int)(bgc->steps % kQSets);
        k.spawn_gate = bgc->launched[k.qpar];
    }
    if (k.fused && g_fused) return launch_fused(k, st, actions, o, sm);
    hipEvent_t fork_ev = nullptr;
    int rc = launch_logic(k, st, actions, o, bgc, fork_ev, sm);
    if (rc) return rc;
    if (k.autoreset == 2) {   // every env resets (the resets write the obs), then the
                              // encodes of the envs rejected for an invalid action
        const KArgs a{k, st, o, nullptr};
        TimedLaunch t2("k_autoreset", sm);
        pick<0, 1>(k.link_in_lds ? 1 : 0, [&](auto jl) {
            pick<4, 8, 16>(lanes_per_env(k.S), [&](auto ms) {
                slaunch((k_autoreset<PICKED(ms), true, PICKED(jl)>), dim3(k.reset_slots), dim3(kWave), k.lds_bytes, sm, a);
            });
        });
        t2.close();
        if ((rc = launch_status("k_autoreset"))) return step_fail(k, st, bgc, false, sm, rc);
        return launch_encode(k, st, o, sm);
    }
    if (!k.autoreset) return launch_encode(k, st, o, sm);
    if (bgc && (rc = launch_spawn(k, st, o, bgc, fork_ev, sm))) return rc;
    const KArgs a{k, st, o, nullptr};
    const PostShape shape = post_shape(k);
    TimedLaunch t2("k_post", sm);
    launch_post(a, shape, k.bg != 0, link_record(k), sm);
    t2.close();
    if ((rc = launch_status("k_post"))) return step_fail(k, st, bgc, bgc != nullptr, sm, rc);
#ifdef SNAKE_DIAG_ENC2
    // Diagnostic timing build: k_post once more with idle workers (aux set), so
    // the encodes alone are timed ("k_encode") with the same launch shape, LDS
    // and registers; they rewrite the same observations.
    if (!k.lean) {
        const KArgs a2{k, st, o, (const void *)1};
        TimedLaunch t5("k_encode", sm);
        launch_post(a2, shape, false, k.link32 ? 2 : 1, sm);
        t5.close();
    }
#endif
    return SNAKE_OK;
}

}  // namespace snake

extern "C" int snake_timing_enable(int on)
{
    std::lock_guard<std::mutex> g(snake::g_tmu);
    snake::g_timing = on != 0;
    return SNAKE_OK;
}

extern "C" int snake_debug_set(const char *name, long long value)
{
    if (name && value >= 0 && value <= INT_MAX) {
        std::lock_guard<std::mutex> g(snake::g_tmu);
        if (!strcmp(name, "draw_wait_ticks")) { snake::g_draw_wait_ticks = (int)value; return SNAKE_OK; }
        if (!strcmp(name, "spawn_delay_ticks")) { snake::g_spawn_delay_ticks = (int)value; return SNAKE_OK; }
        if (!strcmp(name, "fuse_roles")) { snake::g_fuse_roles = (int)value; return SNAKE_OK; }
        if (!strcmp(name, "fused")) { snake::g_fused = value ? 1 : 0; return SNAKE_OK; }
    }
    snake::set_error("snake_debug_set: unknown knob or value out of range");
    return SNAKE_E_ARG;
}

extern "C" int snake_timing_read(const char *kernel, double *total_ms, int64_t *count)
{
    if (!kernel || !total_ms || !count) {
        snake::set_error("snake_timing_read: NULL argument");
        return SNAKE_E_ARG;
    }
    const snake::DiagCounter *dc = nullptr;
    for (const snake::DiagCounter &x : snake::kDiagCounters)
        if (!strcmp(kernel, x.name)) dc = &x;
    if (dc) {
        const void *sym = dc->sym;
        const int n = dc->words;
        std::vector<unsigned long long> v(n, 0ull), z(n, 0ull);
        if (hipMemcpyFromSymbol(v.data(), sym, n * sizeof(unsigned long long)) != hipSuccess ||
            hipMemcpyToSymbol(sym, z.data(), n * sizeof(unsigned long long)) != hipSuccess) {
            snake::set_error("snake_timing_read: reading the reset counter failed");
            return SNAKE_E_LAUNCH;
        }
        unsigned long long t = 0;
        for (unsigned long long x : v) t += x;
        *total_ms = 0.0;
        *count = (int64_t)t;
        return SNAKE_OK;
    }
    std::lock_guard<std::mutex> g(snake::g_tmu);
    for (const auto &r : snake::g_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) {
            snake::set_error("snake_timing_read: event query failed");
            return SNAKE_E_LAUNCH;
        }
        auto &d = snake::g_done[r.name];
        d.first += ms;
        d.second += 1;
        snake::g_pool.push_back(r.a);
        snake::g_pool.push_back(r.b);
    }
    snake::g_pending.clear();
    auto it = snake::g_done.find(kernel);
    *total_ms = it == snake::g_done.end() ? 0.0 : it->second.first;
    *count = it == snake::g_done.end() ? 0 : it->second.second;
    if (it != snake::g_done.end()) snake::g_done.erase(it);
    return SNAKE_OK;
}
