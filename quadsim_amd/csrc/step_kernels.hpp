// step_kernels.hpp -- StepArgs, the tile / obs / counter I/O helpers, the env step kernels, the reset / fill / state I/O kernels
// A fragment of quadsim_hip.hip (ONE translation unit: the kernels' mangled names, which the private-queue code resolves
// in the code object, live in that unit's anonymous namespace); included there at a fixed position, nowhere else.
#pragma once

namespace {

#ifndef QS_BLOCK
#define QS_BLOCK 256
#endif
constexpr int kBlock = QS_BLOCK;  // 4 wavefronts = 4 tiles per workgroup
// Where the rocRAND reset of a step is prepared in the role-split step kernel -- template parameter PREP of k_env_split, chosen
// per launch by the host (bit-identical either way):
//   0  the target wave hands over the Philox words, the chaser wave expands them inside its reset branch (0.6 us of its critical
//      path in 4 workgroups of 5: >= 1 of 64 lanes resets);
//   2  a THIRD wave per workgroup does the draw and the preparation (state, its observation, per-episode params -> LDS), every
//      step, and touches nothing else: the chaser wave's branch is a 25-word LDS copy and the target wave draws nothing.  Every
//      SIMD hosts one wave of each role (tools/wave_map3.hip) at less than half of its issue rate, so the third wave's ~370
//      instructions run beside the others: 65 536 envs 5.05 -> 4.71 us per step (one private queue), 4.6 -> 4.05 us (two),
//      HIP stream 6.6 -> 6.25 us; 32 768 envs 4.31 -> 3.76 us.
//   (1, the TARGET wave preparing it, was measured slower -- it becomes the long pole at barrier #2 -- and is gone.)
// The third wave needs residency: 112 VGPRs allow 4 waves per SIMD, i.e. 4 096 waves on the chip; a launch whose tiles x 3 waves
// exceed that runs its workgroups in two rounds (131 072 envs in ONE launch: 8.9 -> 10.7 us), so PREP = 2 is used up to
// kPrepMaxTiles tiles per launch (QS_RESET_PREP=0/2 forces one; profiles/r03/ab_experiments.txt section J).
#ifndef QS_PREP_MAX_TILES
#define QS_PREP_MAX_TILES 1365
#endif
constexpr int64_t kPrepMaxTiles = QS_PREP_MAX_TILES;
#ifndef QS_SPLIT_MAX_ENVS
#define QS_SPLIT_MAX_ENVS 131072
#endif
constexpr int64_t kSplitMaxEnvs = QS_SPLIT_MAX_ENVS;

struct StepArgs {
    float *st;             // [tiles][40][64]
    float *par;            // [tiles][4][64]
    const float *actions;  // [N,4] (step) / [T,N,4] (rollout) / nullptr (in-kernel random)
    float *obs;            // [N,12] / [T,N,12]
    float *reward;         // [N] / [T,N]
    uint8_t *done;
    uint8_t *flags;        // nullable
    float *term_obs;       // nullable, [N,12] (T == 1 only)
    float *term_state;     // nullable, [N,26] (T == 1 only): chaser 13 | target 13 of the terminal step (docking_env.py:226-229)
    float *slab;           // nullable: packed roll-out slab [T,N,14] = obs 12, reward, done (as 0/1); replaces obs/reward/done
    int64_t n;
    int64_t tile0, tile_end;   // tiles [tile0, tile_end) are stepped by this launch (an env group; the whole handle by default)
    int64_t dbg_shift;         // diagnostic (tests): workgroup b steps tile (b + dbg_shift) % tiles of its launch, i.e. on ANOTHER XCD
    int64_t io_env0, io_n;     // the I/O arrays start at env io_env0 and hold io_n envs per step (0, n: full-batch arrays)
    int64_t T;             // rollout length (1 for step)
    uint64_t step_idx;     // explicit step index (k_fill_actions); the env kernels read the device counter below
    unsigned long long *ctr;   // device: global step counter k, one copy per tile [tiles]
    uint64_t gid0;         // global id of env 0
    EnvConst C;
    RandCfg rc;
    Par par_nom;
    int auto_reset;
    int randomise;
    float nominal_obs[12]; // state2rel of the nominal reset states (what a non-randomised reset returns)
    const float *init;     // stored per-env initial states: [N][26] (docking: chaser, target) / [N][13] (hovering)
    // private-queue launches (qs_set_queue_mode): the launch carries no release fence, so a tile's state stays dirty in the L2 of
    // the XCD that stepped it; `owner` [tiles] records that XCD and every workgroup checks that it runs where its tile lives
    unsigned *owner;       // nullptr: ordinary (fenced) launch, no check.  One 32-bit word per tile, 0xffffffff = unowned;
                           // written and read with agent-scope atomics ONLY: like the state it guards, a plainly stored owner
                           // would stay dirty in the writing XCD's L2 and a misplaced workgroup would never see it
    unsigned *err;         // device word: bit 0 set when a workgroup found its tile owned by another XCD (it then touches nothing)
    unsigned long long *stamps;        // QS_STAMP builds: in-kernel timeline buffer (qs_debug_set_stamps), else nullptr
    unsigned long long stamp_cap, stamp_tiles;
};

__device__ __forceinline__ void load_env(const float *__restrict__ st, int64_t tile, int lane, Env &e)
{
    const float *b = st + tile * (int64_t)(kRecWords * kTile) + lane;
#pragma unroll
    for (int i = 0; i < 13; ++i) e.sc[i] = b[(F_SC + i) * kTile];
#pragma unroll
    for (int i = 0; i < 13; ++i) e.st[i] = b[(F_ST + i) * kTile];
#pragma unroll
    for (int i = 0; i < 4; ++i) e.uc[i] = b[(F_UC + i) * kTile];
#pragma unroll
    for (int i = 0; i < 4; ++i) e.ut[i] = b[(F_UT + i) * kTile];
#pragma unroll
    for (int i = 0; i < 4; ++i) e.qd[i] = b[(F_QD + i) * kTile];
    e.ls = b[F_LS * kTile];
    e.t = b[F_T * kTile];
}

// a wave that needs all 64 lanes (MFMA) on a tail tile: its idle lanes carry a nominal env and store nothing
__device__ __forceinline__ void load_env_or_nominal(const StepArgs &A, int64_t tile, int lane, bool active, Env &e)
{
    if (active) load_env(A.st, tile, lane, e);
    else { nominal_init(e.sc, e.st); for (int i = 0; i < 4; ++i) { e.uc[i] = 0.0f; e.ut[i] = 0.0f; e.qd[i] = i == 0; } e.ls = 0.0f; e.t = 0.0f; }
}

__device__ __forceinline__ void store_env(float *__restrict__ st, int64_t tile, int lane, const Env &e)
{
    float *b = st + tile * (int64_t)(kRecWords * kTile) + lane;
#pragma unroll
    for (int i = 0; i < 13; ++i) QS_ST(&b[(F_SC + i) * kTile], e.sc[i]);
#pragma unroll
    for (int i = 0; i < 13; ++i) QS_ST(&b[(F_ST + i) * kTile], e.st[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) QS_ST(&b[(F_UC + i) * kTile], e.uc[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) QS_ST(&b[(F_UT + i) * kTile], e.ut[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) QS_ST(&b[(F_QD + i) * kTile], e.qd[i]);
    QS_ST(&b[F_LS * kTile], e.ls);
    QS_ST(&b[F_T * kTile], e.t);
}

__device__ __forceinline__ Par load_par(const float *__restrict__ par, int64_t tile, int lane)
{
    const float *b = par + tile * (int64_t)(kParWords * kTile) + lane;
    Par P;
    P.m = b[0]; P.Ixx = b[kTile]; P.Iyy = b[2 * kTile]; P.Izz = b[3 * kTile];
    return P;
}

__device__ __forceinline__ void store_par(float *__restrict__ par, int64_t tile, int lane, const Par &P)
{
    float *b = par + tile * (int64_t)(kParWords * kTile) + lane;
    b[0] = P.m; b[kTile] = P.Ixx; b[2 * kTile] = P.Iyy; b[3 * kTile] = P.Izz;
}

// the wave prologue of a kernel that gives every wave of its kBlock-thread workgroups one tile of a whole-handle launch:
// this lane, its tile, its env, and whether that env exists (env < n)
struct TileLane { int lane; int64_t tile, env; bool active; };
__device__ __forceinline__ TileLane tile_lane(int64_t n)
{
    const int lane = threadIdx.x & (kTile - 1);
    const int64_t tile = (int64_t)blockIdx.x * (kBlock / kTile) + (threadIdx.x >> 6);
    const int64_t env = tile * kTile + lane;
    return {lane, tile, env, env < n};
}

__device__ __forceinline__ void store_obs(float *__restrict__ obs, int64_t env, const float o[12])
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 *p = reinterpret_cast<f4 *>(obs + env * 12);
    QS_SO(&p[0], (f4{o[0], o[1], o[2], o[3]}));
    QS_SO(&p[1], (f4{o[4], o[5], o[6], o[7]}));
    QS_SO(&p[2], (f4{o[8], o[9], o[10], o[11]}));
}

// plain (cached) flavour: rows that are completed by LATER stores of the same lane (the env-major roll-out arrays, where a
// lane's consecutive steps fill consecutive slots of one line) should stay in the L2 until they are whole
__device__ __forceinline__ void store_obs_cached(float *__restrict__ obs, int64_t env, const float o[12])
{
    float4 *p = reinterpret_cast<float4 *>(obs + env * 12);
    p[0] = make_float4(o[0], o[1], o[2], o[3]);
    p[1] = make_float4(o[4], o[5], o[6], o[7]);
    p[2] = make_float4(o[8], o[9], o[10], o[11]);
}

// one env.step for the lane's env + VecEnv auto-reset; shared by step and rollout kernels
// The global step counter k lives in device memory so that a captured launch (hipGraph / torch.cuda.graphs) advances
// it on every replay.  It is kept PER TILE (one 64-bit word per wavefront's tile; all tiles hold the same value):
// a wave reads its own word at the start and writes k + T back at the end, so no workgroup ever waits for or
// races with another one.  (A single shared word updated through a per-workgroup ticket cost 2 us per launch.)
__device__ __forceinline__ uint64_t step_counter_begin(const StepArgs &A, int64_t tile) { return A.ctr[tile]; }
// The single-step kernels request the word through the vector memory path (the zero below hides the wave-uniform address from
// the compiler): as a scalar load it shared one counter -- and one wait -- with the kernel-argument fetch in front of the state
// loads, i.e. an L2 round trip on every wave's critical path; as a vector load it is one more load beside the state's
// (nominal-reset kernel 4.87 -> 4.74 us per step, two queues 4.41 -> 4.16; section J15)
__device__ __forceinline__ uint64_t step_counter_begin_vmem(const StepArgs &A, int64_t tile)
{
    int zero;
    asm("v_mov_b32 %0, 0" : "=v"(zero));
    return A.ctr[tile + zero];
}
__device__ __forceinline__ void step_counter_end(const StepArgs &A, int64_t tile, int lane, uint64_t k)
{
    if (lane == 0) A.ctr[tile] = k + (uint64_t)A.T;
}

// private-queue launches only: true when this wave must not touch its tile (the tile's latest state is in another XCD's L2).
// Blocks are dealt to the XCDs round-robin from a start that is constant for a queue (measured: tools/xcc_map.hip), so this
// never fires; it turns a change of that hardware behaviour into a loud error instead of stale state.
// The owner word is requested with an agent-scope atomic load (`sc1`: never served from a stale line of this XCD's L2 or this
// CU's L1) and claimed with an agent-scope compare-and-swap executed at the memory side: every XCD sees the same word.
constexpr unsigned kUnowned = 0xffffffffu;
__device__ __forceinline__ unsigned chain_owner_request(const StepArgs &A, int64_t tile)
{
    // no control flow around the load (an ordinary launch reads a word of its own step counter instead and ignores it): a
    // load inside a branch is issued late and waited for at the branch's end (section J15)
    const unsigned *p = A.owner ? A.owner + tile : reinterpret_cast<const unsigned *>(A.ctr + tile);
    const unsigned v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return A.owner ? v : kUnowned;
}

// the check for a caller that requested the owner word earlier (no load latency on its critical path)
__device__ __forceinline__ bool chain_owner_mismatch(const StepArgs &A, int64_t tile, int lane, unsigned own)
{
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 15u;   // HW_REG_XCC_ID
    if (own == kUnowned) {
        // first private step of this tile since the handle's last HIP-side call: claim it (both role waves may try; the
        // second one finds its own XCD).  A claim lost to ANOTHER XCD is a misplacement like any other.
        unsigned seen = kUnowned;
        if (lane == 0) {
            unsigned expect = kUnowned;
            __hip_atomic_compare_exchange_strong(&A.owner[tile], &expect, xcc, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            seen = expect;
        }
        own = __builtin_amdgcn_readfirstlane(seen);
        if (own == kUnowned) return false;
    }
    if (own != xcc) {
        if (lane == 0) __hip_atomic_fetch_or(A.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // host memory
        return true;
    }
    return false;
}

__device__ __forceinline__ bool chain_tile_misplaced(const StepArgs &A, int64_t tile, int lane)
{
    if (!A.owner) return false;
    return chain_owner_mismatch(A, tile, lane, chain_owner_request(A, tile));
}

// tile of workgroup-local index b (0 <= b < the launch's tile count); dbg_shift != 0 only in the placement-guard test.
// Branch-free on purpose, with dbg_shift next to tile0 / tile_end in StepArgs: a branch on a kernel argument at the very top of
// the kernel made the compiler fetch that argument, wait, and only then fetch the rest -- a second scalar-memory round trip in
// front of every wave's loads (+0.3 us per step; profiles/r03/ab_experiments.txt section J15).
__device__ __forceinline__ int64_t launch_tile(const StepArgs &A, int64_t b)
{
    const int64_t nt = A.tile_end - A.tile0;
    b += A.dbg_shift;
    b -= (b >= nt) ? nt : 0;
    return A.tile0 + b;
}

template <bool PARAMS, int RMODE>
__device__ __forceinline__ void maybe_reset(Env &e, Par &P, const StepArgs &A, int64_t env, uint64_t k, float obs[12], unsigned flags,
                                            bool &done, bool write_term);

// RMODE (compile time) = the handle's `randomise`: 0 nominal reset, 1 rocRAND init state, 2 + params.
template <int INTEG, bool PARAMS, int RMODE>
__device__ __forceinline__ void step_and_maybe_reset(Env &e, Par &P, const float a[4], const StepArgs &A, int64_t env,
                                                     uint64_t k, float obs[12], float &reward, unsigned &flags,
                                                     bool &done, bool write_term)
{
    env_step<INTEG>(e, a, P, A.C, obs, reward, flags);
    maybe_reset<PARAMS, RMODE>(e, P, A, env, k, obs, flags, done, write_term);
}

template <bool PARAMS, int RMODE>
__device__ __forceinline__ void maybe_reset(Env &e, Par &P, const StepArgs &A, int64_t env, uint64_t k, float obs[12], unsigned flags,
                                            bool &done, bool write_term)
{
    done = (flags & (FLAG_OVERLIMIT | FLAG_OVERTIME)) != 0;
    if (done && A.auto_reset) {
        if (write_term && A.term_obs) store_obs(A.term_obs, env - A.io_env0, obs);
        if (write_term && A.term_state) {
            float *ts = A.term_state + (env - A.io_env0) * 26;
#pragma unroll
            for (int i = 0; i < 13; ++i) { ts[i] = e.sc[i]; ts[13 + i] = e.st[i]; }
        }
        if (RMODE == 0) {
            // nominal states are constants: no need to re-derive their observation per lane
            nominal_init(e.sc, e.st);
#pragma unroll
            for (int i = 0; i < 4; ++i) { e.uc[i] = 0.0f; e.ut[i] = 0.0f; }
            e.ls = 0.0f;
            e.t = 0.0f;
#pragma unroll
            for (int i = 0; i < 12; ++i) obs[i] = A.nominal_obs[i];
        } else if (RMODE == 3) {
            // stored per-env initial state (docking-v1; script-set chaser_ini_state)
            float ic[13], it[13];
            const float *src = A.init + env * 26;
#pragma unroll
            for (int i = 0; i < 13; ++i) { ic[i] = src[i]; it[i] = src[13 + i]; }
            env_reset<false>(e, ic, it, obs);
        } else {
            float ic[13], it[13];
            Par Pn;
            random_init<RMODE == 2>(A.rc, STREAM_AUTORESET, A.gid0 + (uint64_t)env, k + 1, ic, it, Pn);
            if (PARAMS && RMODE == 2) P = Pn;
            env_reset<true>(e, ic, it, obs);   // randomised reset states always have a level target
        }
    }
}

// K1/K4: T fused env.steps for N envs in one launch, env state in registers between the tile load
// and the tile store.  T == 1 is DockingEnv.step (docking_env.py:104-231); T > 1 is the trainer's
// Runner loop (rl_baselines/ppo2/ppo2.py:472-499) with the actions pre-staged or drawn in-kernel.
// One kernel serves both so that a roll-out is bit-identical to T single steps (same machine code).
template <int INTEG, bool PARAMS, int RMODE>
__global__ __launch_bounds__(kBlock) void k_env(StepArgs A)
{
    const int lane = threadIdx.x & (kTile - 1);
    const int64_t wg_tile = (int64_t)blockIdx.x * (kBlock / kTile) + (threadIdx.x >> 6);
    if (wg_tile >= A.tile_end - A.tile0) return;
    const int64_t tile = launch_tile(A, wg_tile);
    const int64_t env = tile * kTile + lane;
    if (env >= A.n) return;
    if (chain_tile_misplaced(A, tile, lane)) return;
    const int64_t io = env - A.io_env0;          // row of this env in the I/O arrays
    QS_ASSERT(io >= 0 && io < A.io_n);
    const uint64_t k0 = step_counter_begin_vmem(A, tile);
    // the first action is requested together with the tile (one exposed memory latency per launch, not two) and
    // every later one a whole step ahead of its use
    float4 av_next = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (A.actions) av_next = reinterpret_cast<const float4 *>(A.actions)[io];
    Env e;
    load_env(A.st, tile, lane, e);
    Par P = A.par_nom;
    if (PARAMS) P = load_par(A.par, tile, lane);
#pragma clang loop unroll(disable)
    for (int64_t t = 0; t < A.T; ++t) {
        const uint64_t k = k0 + (uint64_t)t;
        const int64_t o = t * A.io_n + io;
        float a[4];
        if (A.actions) {
            const float4 av = av_next;
            if (t + 1 < A.T) av_next = reinterpret_cast<const float4 *>(A.actions)[o + A.io_n];
            a[0] = av.x; a[1] = av.y; a[2] = av.z; a[3] = av.w;
        } else {
            random_action(A.rc.seed, A.gid0 + (uint64_t)env, k, a);
        }
        float obs[12], reward;
        unsigned flags;
        bool done;
        step_and_maybe_reset<INTEG, PARAMS, RMODE>(e, P, a, A, env, k, obs, reward, flags, done, true);
        if (A.slab) {
            // one 56-byte row per env-step (the unit the multi-GPU all-gather moves): seven 8-byte stores
            float2 *row = reinterpret_cast<float2 *>(A.slab + o * 14);
#pragma unroll
            for (int i = 0; i < 6; ++i) row[i] = make_float2(obs[2 * i], obs[2 * i + 1]);
            row[6] = make_float2(reward, done ? 1.0f : 0.0f);
        } else {
            store_obs(A.obs, o, obs);
            QS_SO(&A.reward[o], reward);
            QS_SO(&A.done[o], (uint8_t)(done ? 1 : 0));
        }
        if (A.flags) QS_SO(&A.flags[o], (uint8_t)flags);
    }
    store_env(A.st, tile, lane, e);
    if (PARAMS && RMODE == 2) store_par(A.par, tile, lane, P);
    step_counter_end(A, tile, lane, k0);
}

// Role-split variant of k_env: one workgroup = one tile = TWO waves.  Wave 0 carries the chaser side of the 64 envs (action
// mix, chaser drone step, state2rel, reward, done, the chaser's reset), wave 1 the target side (target drone step, the
// target's PID, the rocRAND draw a reset of this step would consume).  A lone wave issues a vector instruction every 4
// cycles and two waves on a SIMD every 2 each (MI355X_MICROARCH.md), so at one tile per SIMD the two half-length
// instruction streams run in the time of one.  Hand-overs through 7.5 KiB of LDS, two workgroup barriers per step:
//   target wave:  advance target | draw Philox words  -> #1 ->  PID, limit new control            -> #2 -> apply reset
//   chaser wave:  mix, advance chaser                 -> #1 ->  state2rel, reward, done -> flag  -> #2 -> reset, stores
// waves per workgroup of k_env_split: with PREP == 2 the rocRAND reset modes get a third wave
constexpr int split_waves(int rmode, int prep) { return (prep == 2 && (rmode == 1 || rmode == 2)) ? 3 : 2; }

// ---- the step body shared by k_env_split and k_env_resident ----------------------------------------------------------------
// Everything a role wave computes in a step is one of the functions below; the two kernels differ in what surrounds them (loop
// control, where a step's I/O pointers come from, the placement guard, s_setprio) and own every workgroup barrier: none of
// these functions contains one.

// LDS of a workgroup; an array that the instantiation does not use has no rows, so that it takes no LDS.
// rst (third wave): [chaser reset state 13 | its observation 12 | per-episode params 4][lane]: what a reset of THIS step would
// install, prepared every step off the chaser wave's critical path.  One buffer suffices in a roll-out too: it is written
// between barriers #1 and #2 of a step and read behind #2; the next write is behind the NEXT step's #1, which the readers have
// passed.  phx (rocRAND reset modes without the third wave): [step parity][block]: the chaser wave reads step t's Philox words
// while t+1's are drawn.
constexpr bool split_prep(int rmode, int prep) { return split_waves(rmode, prep) == 3; }
constexpr bool split_draw(int rmode, int prep) { return (rmode == 1 || rmode == 2) && !split_prep(rmode, prep); }
template <int RMODE, int PREP>
struct SplitLds {
    float tgt[13][kTile];
    float rst[split_prep(RMODE, PREP) ? 29 : 0][kTile];
    uint4 phx[split_draw(RMODE, PREP) ? 2 : 0][2][kTile];
    unsigned char done[kTile], limt[kTile];
    __device__ __forceinline__ Par reset_par(int lane) const { return Par{rst[25][lane], rst[26][lane], rst[27][lane], rst[28][lane]}; }
};

__device__ __forceinline__ void chaser_load(const float *b, float sc[13], float uc[4], float &ls, float &tt)
{
#pragma unroll
    for (int i = 0; i < 13; ++i) sc[i] = b[(F_SC + i) * kTile];
#pragma unroll
    for (int i = 0; i < 4; ++i) uc[i] = b[(F_UC + i) * kTile];
    ls = b[F_LS * kTile];
    tt = b[F_T * kTile];
}

__device__ __forceinline__ void chaser_store(float *bw, const float sc[13], const float uc[4], float ls, float tt)
{
#pragma unroll
    for (int i = 0; i < 13; ++i) QS_ST(&bw[(F_SC + i) * kTile], sc[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) QS_ST(&bw[(F_UC + i) * kTile], uc[i]);
    QS_ST(&bw[F_LS * kTile], ls);
    QS_ST(&bw[F_T * kTile], tt);
}

// chaser wave between #1 and #2: state2rel against the target's new state, reward, flags; -> this lane resets (also into LDS)
template <int RMODE, int PREP>
__device__ __forceinline__ bool chaser_score(SplitLds<RMODE, PREP> &L, int lane, const float sc[13], const float a[4], float tt, float &ls,
                                             const EnvConst &C, int auto_reset, bool lim_c, float obs[12], float &reward,
                                             unsigned &flags, bool &done)
{
    float st[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) st[i] = L.tgt[i][lane];
    const bool lim_t = L.limt[lane] != 0;
    rel_obs(sc, st, obs);
    score_step(obs, a, sc[2], tt, ls, C, lim_c, lim_t, reward, flags);
    done = (flags & (FLAG_OVERLIMIT | FLAG_OVERTIME)) != 0;
    const bool rs = done && auto_reset;
    L.done[lane] = rs ? 1 : 0;
    return rs;
}

// one drone's half (0 chaser, 1 target) of a terminal-state row
__device__ __forceinline__ void store_term_half(float *term_state, bool active, int64_t io, int half, const float s[13])
{
    if (term_state && active) {
        float *ts = term_state + io * 26 + 13 * half;
#pragma unroll
        for (int i = 0; i < 13; ++i) ts[i] = s[i];
    }
}

// the chaser's half of an auto-reset, behind #2: new state, its observation, the episode's parameters
template <bool PARAMS, int RMODE, int PREP>
__device__ __forceinline__ void chaser_reset(const SplitLds<RMODE, PREP> &L, const StepArgs &A, int64_t env, bool active, int lane, int64_t t,
                                             float sc[13], float uc[4], float &ls, float &tt, Par &P, float obs[12])
{
    float ic[13], it[13];
    if (RMODE == 0) {
        nominal_init(ic, it);
#pragma unroll
        for (int i = 0; i < 12; ++i) obs[i] = A.nominal_obs[i];
    } else if (RMODE == 3) {
        const float *src = A.init + (active ? env : 0) * 26;
#pragma unroll
        for (int i = 0; i < 13; ++i) { ic[i] = src[i]; it[i] = src[13 + i]; }
        rel_obs<false>(ic, it, obs);
    } else {
        if constexpr (split_prep(RMODE, PREP)) {
            // the reset state, its observation and the episode's parameters were prepared by the third wave: a copy
#pragma unroll
            for (int i = 0; i < 13; ++i) ic[i] = L.rst[i][lane];
#pragma unroll
            for (int i = 0; i < 12; ++i) obs[i] = L.rst[13 + i][lane];
            if (PARAMS && RMODE == 2) P = L.reset_par(lane);
        } else {
            const uint4 w0 = L.phx[t & 1][0][lane], w1 = RMODE == 2 ? L.phx[t & 1][1][lane] : make_uint4(0, 0, 0, 0);
            Par Pn;
            random_init_apply<RMODE == 2>(A.rc, w0, w1, ic, it, Pn);
            if (PARAMS && RMODE == 2) P = Pn;
            rel_obs<true>(ic, it, obs);
        }
    }
#pragma unroll
    for (int i = 0; i < 13; ++i) sc[i] = ic[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) uc[i] = 0.0f;
    ls = 0.0f;
    tt = 0.0f;
}

__device__ __forceinline__ void target_load(const float *b, float st[13], float ut[4], float qd[4])
{
#pragma unroll
    for (int i = 0; i < 13; ++i) st[i] = b[(F_ST + i) * kTile];
#pragma unroll
    for (int i = 0; i < 4; ++i) ut[i] = b[(F_UT + i) * kTile];
#pragma unroll
    for (int i = 0; i < 4; ++i) qd[i] = b[(F_QD + i) * kTile];
}

__device__ __forceinline__ void target_store(float *bw, const float st[13], const float ut[4], const float qd[4])
{
#pragma unroll
    for (int i = 0; i < 13; ++i) QS_ST(&bw[(F_ST + i) * kTile], st[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) QS_ST(&bw[(F_UT + i) * kTile], ut[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) QS_ST(&bw[(F_QD + i) * kTile], qd[i]);
}

// target wave before #1: the advanced target -> LDS; without the third wave also the Philox words a reset of this step consumes
template <int RMODE, int PREP>
__device__ __forceinline__ void target_publish(SplitLds<RMODE, PREP> &L, const StepArgs &A, int64_t env, int lane, uint64_t k, int64_t t,
                                               const float st[13], bool lim_t, uint4 &w0, uint4 &w1)
{
#pragma unroll
    for (int i = 0; i < 13; ++i) L.tgt[i][lane] = st[i];
    L.limt[lane] = lim_t ? 1 : 0;
    w0 = make_uint4(0, 0, 0, 0);
    w1 = w0;
    if constexpr (split_draw(RMODE, PREP)) {
        random_init_words<RMODE == 2>(A.rc, STREAM_AUTORESET, A.gid0 + (uint64_t)env, k + 1, w0, w1);
        L.phx[t & 1][0][lane] = w0;
        if (RMODE == 2) L.phx[t & 1][1][lane] = w1;     // the params block: only drawn with per-episode params
    }
}

// target wave between #1 and #2: the PID from the state BEFORE stepping, and the new limited control
__device__ __forceinline__ void target_command(const EnvConst &C, float qd[4], const float pre[13], float m, float ut[4])
{
    const float pdes[3] = {10.0f, -50.0f, 5.0f};              // docking_env.py:60
    const float vdes[3] = {C.vdes_x, 0.0f, 0.0f};
    const float dv[3] = {0.0f, 0.0f, 0.0f};
    float u_t[4];
    target_control(C.kind, pdes, vdes, qd, 0.0f, pre, dv, m, u_t);
    u_limit(u_t, m * kG, ut);
}

// the target's half of an auto-reset, behind #2 (w0, w1: this step's words from target_publish)
template <bool PARAMS, int RMODE, int PREP>
__device__ __forceinline__ void target_reset(const SplitLds<RMODE, PREP> &L, const StepArgs &A, int64_t env, bool active, int lane,
                                             const uint4 &w0, const uint4 &w1, float st[13], float ut[4], Par &P)
{
    float ic[13], it[13];
    if (RMODE == 3) {
        const float *src = A.init + (active ? env : 0) * 26;
#pragma unroll
        for (int i = 0; i < 13; ++i) it[i] = src[13 + i];
    } else {
        nominal_init(ic, it);
        if (PARAMS && RMODE == 2) {
            if constexpr (split_prep(RMODE, PREP)) {
                P = L.reset_par(lane);
            } else {
                random_init_apply<true>(A.rc, w0, w1, ic, it, P);
                nominal_init(ic, it);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 13; ++i) st[i] = it[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) ut[i] = 0.0f;
}

// third wave (rocRAND reset modes with PREP == 2 only) between #1 and #2: what a reset of this step would install --
// random_init_apply on the words it drew before #1 and the state2rel of the result: the same device functions the serial kernel
// runs inside its reset branch, so the same bits -- for EVERY lane, into LDS.  The wave touches no global memory but the step
// counter and joins both barriers of every step; the chaser wave's reset branch is a 25-word copy, the target wave draws nothing.
template <bool PARAMS, int RMODE, int PREP>
__device__ __forceinline__ void prep_publish(SplitLds<RMODE, PREP> &L, const RandCfg &rc, int lane, const uint4 &w0, const uint4 &w1)
{
    float ic[13], it_[13], robs[12];
    Par Pn;
    random_init_apply<RMODE == 2>(rc, w0, w1, ic, it_, Pn);
    rel_obs<true>(ic, it_, robs);
#pragma unroll
    for (int i = 0; i < 13; ++i) L.rst[i][lane] = ic[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) L.rst[13 + i][lane] = robs[i];
    if (PARAMS && RMODE == 2) {
        L.rst[25][lane] = Pn.m; L.rst[26][lane] = Pn.Ixx; L.rst[27][lane] = Pn.Iyy; L.rst[28][lane] = Pn.Izz;
    }
}

// ---- resident form of k_env_split (host-ordered private queues; private_queue.hpp, "resident roll-out") -------------------
// One dispatch per private queue steps its tiles for as many steps as the host issues.  Before each step the chaser wave takes
// that step's I/O pointers from a descriptor ring the host writes ahead of the GPU; the state stays in registers from one step
// to the next and is stored once, when the tile leaves.  A step is k_env_split's: the same calls of the shared step body above.
//
// A descriptor is 8 naturally aligned 64-bit words (one 64-B slot): actions | obs | reward | done | flags | term_obs |
// term_state | command.  EVERY word carries the low 16 bits of the step's sequence number (the tag) in bits 48..63, beside a
// 48-bit pointer; the command word also holds sequence bits 16..47 in its bits 0..31.  Slot s % slots holds step s.
//   - Torn slot: each word is single-copy atomic (an aligned 8-byte store on the host, an 8-byte atomic load here) and
//     validates itself: a word of another lap carries another tag.  No ordering between the words is needed.
//   - Stale slot: the host rewrites a slot only after every tile has consumed it, so memory holds the current or the previous
//     lap; a slot of an earlier lap served from some cache carries an older sequence number in the command word (32 more bits),
//     so it never passes for a fresh one.  A slot that is not fresh is polled again (system-scope loads, s_sleep between them)
//     until it is or until the idle limit: a wrong descriptor -- a wild pointer -- is never used.
constexpr int kResWords = 8;
constexpr unsigned long long kResPtrMask = (1ull << 48) - 1;
enum { RES_STEP = 0, RES_EXIT = 1, RES_IDLE = 2, RES_SKIP = 3 };
// Progress: every tile reports once per kResWin descriptors (staggered by tile % kResWin, so ~tiles / kResWin agent-scope adds
// per step, not one per tile) into window counter (s - base + tile % kResWin + 1) / kResWin, counted from the roll-out's first
// descriptor `base` so that every window receives one report from every tile; the tile whose add completes a window writes
// ONE host word: every tile of the dispatch has consumed every descriptor before it.  The host reuses slots by it.
constexpr int kResWin = 32;
constexpr int kResWinSlots = 16;     // > slots / kResWin + 2 windows in flight (the host checks)

struct ResArgs {
    const unsigned long long *ring;   // [slots][8] descriptors: device memory the host writes through the PCIe BAR
    unsigned long long *rseq;         // [tiles] next descriptor of each tile (written when the tile leaves)
    unsigned *wcnt;                   // [kResWinSlots] this dispatch's window counters (zeroed by the host per roll-out)
    unsigned *fin;                    // this dispatch's count of tiles that consumed the EXIT descriptor (zeroed likewise)
    unsigned long long *h_prog;       // host word: descriptors below it are consumed by every tile of the dispatch
    unsigned long long *h_fin;        // host word: EXIT seq + 1 once every tile of the dispatch has consumed the EXIT
    unsigned long long seq0;          // != 0: every tile starts at seq0 (first dispatch of a roll-out), else at rseq[tile]
    unsigned long long base;          // the roll-out's first descriptor (progress windows count from it)
    unsigned long long stop_seq;      // a tile whose next descriptor is >= stop_seq ends at once (relaunch after an EXIT)
    unsigned long long slots_mask;    // slots - 1
    unsigned long long idle_ticks;    // 100 MHz ticks without a fresh descriptor after which a tile stores its state and ends
    unsigned lane_tiles;              // tiles of this dispatch
};

struct ResDesc {
    const float *actions;
    float *obs, *reward;
    uint8_t *done, *flags;
    float *term_obs, *term_state;
};

// lanes 0..7 (and their copies above) each request one word of slot s: one 64-B request, system scope (never an L1 line)
__device__ __forceinline__ unsigned long long res_request(const ResArgs &R, unsigned long long s, int lane)
{
    return __hip_atomic_load(R.ring + (s & R.slots_mask) * kResWords + (lane & 7), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ bool res_fresh(unsigned long long w, unsigned long long s, int lane)
{
    bool ok = (w >> 48) == (s & 0xffffull);
    if ((lane & 7) == 7) ok = ok && (unsigned)w == (unsigned)(s >> 16);
    return __all(ok);
}

__device__ __forceinline__ unsigned long long res_word(unsigned long long w, int i)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)w, i);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(w >> 32), i);
    return (((unsigned long long)hi << 32) | lo) & kResPtrMask;
}

// descriptor s from the word `w` requested earlier, polled again until fresh or for at most R.idle_ticks
__device__ __forceinline__ int res_resolve(const ResArgs &R, unsigned long long s, int lane, unsigned long long w, ResDesc &D)
{
    if (!res_fresh(w, s, lane)) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            __builtin_amdgcn_s_sleep(4);
            w = res_request(R, s, lane);
            if (res_fresh(w, s, lane)) break;
            if (__builtin_amdgcn_s_memrealtime() - t0 > R.idle_ticks) return RES_IDLE;
        }
    }
    D.actions = (const float *)res_word(w, 0);
    D.obs = (float *)res_word(w, 1);
    D.reward = (float *)res_word(w, 2);
    D.done = (uint8_t *)res_word(w, 3);
    D.flags = (uint8_t *)res_word(w, 4);
    D.term_obs = (float *)res_word(w, 5);
    D.term_state = (float *)res_word(w, 6);
    return ((res_word(w, 7) >> 32) & 0xff) == 0 ? RES_STEP : RES_EXIT;
}

// the action row of step descriptor D: a system-scope (`sc0 sc1`) buffer load -- the caller may have rewritten the same
// buffer since an earlier step of this dispatch, so no L1 or stale L2 line may serve it; rows past io_n read as zeros
__device__ __forceinline__ float4 res_action(const float *actions, int64_t io, int64_t io_n)
{
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)actions, (short)0, (int)(io_n * 16), 0x00020000);
    const u4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(io * 16), 0, 17);   // cache policy 17: sc0 sc1
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// store_obs and store_term_half through descriptor pointers: the same stores, global-addressed (kernel_diag.hpp, QS_GLOBAL_PTR)
__device__ __forceinline__ void res_store_obs(float *obs, int64_t env, const float o[12])
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    QS_GLOBAL f4 *p = QS_GLOBAL_PTR(f4, obs + env * 12);
    QS_SO(&p[0], (f4{o[0], o[1], o[2], o[3]}));
    QS_SO(&p[1], (f4{o[4], o[5], o[6], o[7]}));
    QS_SO(&p[2], (f4{o[8], o[9], o[10], o[11]}));
}

__device__ __forceinline__ void res_store_term_half(float *term_state, bool active, int64_t io, int half, const float s[13])
{
    if (term_state && active) {
        QS_GLOBAL float *ts = QS_GLOBAL_PTR(float, term_state + io * 26 + 13 * half);
#pragma unroll
        for (int i = 0; i < 13; ++i) ts[i] = s[i];
    }
}

// lane 0, after consuming step descriptor s: the tile's report into its progress window, if s closes one (wave-uniform);
// returns the counter's previous value, checked by res_report_done once the add has long returned
__device__ __forceinline__ unsigned res_report(const ResArgs &R, unsigned long long s, int64_t tile, int lane)
{
    const unsigned long long x = s - R.base + (unsigned long long)(tile % kResWin) + 1;
    if (x % kResWin != 0) return ~0u;
    unsigned old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(R.wcnt + (x / kResWin) % kResWinSlots, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return old;
}

__device__ __forceinline__ void res_report_done(const ResArgs &R, unsigned old, unsigned long long s, int64_t tile, int lane)
{
    if (old == ~0u || lane != 0 || (old + 1) % R.lane_tiles != 0) return;
    // the window is complete: every tile consumed its report descriptor, the earliest of them base + x - kResWin
    const unsigned long long x = s - R.base + (unsigned long long)(tile % kResWin) + 1;
    __hip_atomic_store(R.h_prog, R.base + x - kResWin + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// k_env_split's step, taken from the descriptor ring until an EXIT descriptor or the idle limit.  What differs from k_env_split:
// barrier #0 before the first step; the next descriptor is requested at the top of a step and resolved where k_env_split
// requests the next action; a step's I/O pointers are those of its descriptor D; no placement guard and no slab; the chaser
// wave keeps its priority for the whole dispatch; the state is stored once, when the tile leaves.
// Memory waits of the chaser wave: gfx950 counts loads, returning atomics and stores in ONE in-order vmcnt, so a wait for any
// loaded value behind a step's stores is also a wait for their acknowledge, during which the wave issues nothing.  A step
// therefore has one such wait, in FRONT of its first store (res_report_done reads the progress add's result, requested
// before #1 like the next action), and the reset branch only computes: its terminal rows stay in registers until then.  The
// stores of step t drain under drone_advance of step t + 1, up to the wait for descriptor t + 2.  Nothing reads them before
// the dispatch has ended (the host waits for its completion signal, a system-scope release); two steps' stores to one buffer
// come from the same wave in issue order.  The state loads are waited for once, before the loop.
// Full stamp build: stamp 1 is retaken at the top of every step, so that the stamps a tile flushes when it leaves are the
// timeline of its LAST step (1 step start, 2 before #1, 3 after #1, 4 before #2, 5 after #2, 6 / 7 as in k_env_split).
#if defined(QS_STAMP) && QS_STAMP + 0 < 2
#define QS_STAMP_STEP() QS_STAMP_AT(1)
#else
#define QS_STAMP_STEP() ((void)0)
#endif
template <int INTEG, bool PARAMS, int RMODE, int PREP>
__global__ __launch_bounds__(3 * kTile) void k_env_resident(StepArgs A, ResArgs R)
{
    __shared__ SplitLds<RMODE, PREP> L;
    // [step parity] the command and the term_state pointer of step t + 1, written by the chaser wave in step t before #1.
    // The command is read by every wave behind #2 of step t; the next write of that parity is behind two more #1s.  The
    // pointer is read by the target wave between #1 and #2 of step t + 1: the chaser wave rewrites that parity in step t + 2
    // before #1, with no barrier between it and #2 of step t + 1, so a read behind #2 could see step t + 3's pointer.
    __shared__ int s_cmd[2];
    __shared__ unsigned long long s_tsp[2];
    const int lane = threadIdx.x & (kTile - 1);
    const int role = threadIdx.x >> 6;
    const int64_t tile = launch_tile(A, blockIdx.x);   // grid = the tiles of this launch's env group
    const int64_t env = tile * kTile + lane;
    bool active = env < A.n;                     // idle lanes of the tail tile compute on zeros and store nothing
    const int64_t io = env - A.io_env0;          // row of this env in the I/O arrays
    QS_ASSERT(tile < A.tile_end && (!active || (io >= 0 && io < A.io_n)));
    const uint64_t k0 = step_counter_begin_vmem(A, tile);
    // the tile's first descriptor, handed to the other waves behind one extra barrier per dispatch
    unsigned long long seq = 0;
    int cmd = RES_STEP;
    ResDesc D{};
    {
        if (role == 0) {
            seq = R.seq0 ? R.seq0 : R.rseq[tile];
            seq = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(unsigned)(seq >> 32)) << 32) |
                  (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)seq);
            cmd = seq >= R.stop_seq ? RES_SKIP : res_resolve(R, seq, lane, res_request(R, seq, lane), D);
            if (cmd == RES_STEP) res_report_done(R, res_report(R, seq, tile, lane), seq, tile, lane);
            if (lane == 0) { s_cmd[0] = cmd; s_tsp[0] = (unsigned long long)D.term_state; }
        }
        __syncthreads();                                                  // #0
        cmd = s_cmd[0];
    }
    QS_STAMP_DECL;
    QS_STAMP_AT(0);
    const float *b = A.st + tile * (int64_t)(kRecWords * kTile) + lane;
    float *bw = A.st + tile * (int64_t)(kRecWords * kTile) + lane;
    Par P = A.par_nom;
    if (PARAMS) P = load_par(A.par, tile, lane);
    if (role == 0) {
        __builtin_amdgcn_s_setprio(3);           // as k_env_split in a roll-out
        float sc[13], uc[4], ls, tt;
        chaser_load(b, sc, uc, ls, tt);
        // the action is requested LAST, as in k_env_split
        float4 av_next = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (cmd == RES_STEP && active) av_next = res_action(D.actions, io, A.io_n);
#if defined(QS_STAMP) && QS_STAMP + 0 < 2
        asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
#endif
        QS_STAMP_AT(1);
        QS_WAIT_VMEM();                          // the state rows, here and not at the top of every step
        int64_t t = 0;
#pragma clang loop unroll(disable)
        for (; cmd == RES_STEP; ++t) {
            QS_STAMP_STEP();
            const int64_t o = io;
            const unsigned long long wn = res_request(R, seq + t + 1, lane);   // the next descriptor, a step ahead of its use
            tt += 1.0f;
            const bool lim_c = drone_advance<INTEG>(sc, uc, P, A.C.dt);   // Drone.step's integration: previous control only
            float a[4];
            ResDesc Dn{};
            unsigned rep = ~0u;
            const float4 av = av_next;
            const int cmdn = res_resolve(R, seq + t + 1, lane, wn, Dn);
            if (cmdn == RES_STEP) {
                if (active) av_next = res_action(Dn.actions, io, A.io_n);
                rep = res_report(R, seq + t + 1, tile, lane);
            }
            if (lane == 0) { s_cmd[(t + 1) & 1] = cmdn; s_tsp[(t + 1) & 1] = (unsigned long long)Dn.term_state; }
            a[0] = av.x; a[1] = av.y; a[2] = av.z; a[3] = av.w;
            float u_c[4];
            chaser_command(a, P.m, u_c);
            u_limit(u_c, P.m * kG, uc);                                   // ... and the hand-over of the new limited control
            QS_STAMP_AT(2);
            __syncthreads();                                              // #1: the target's new state is in LDS
            QS_STAMP_AT(3);
            float obs[12], reward;
            unsigned flags;
            bool done;
            const bool rs = chaser_score(L, lane, sc, a, tt, ls, A.C, A.auto_reset, lim_c, obs, reward, flags, done);
            QS_STAMP_AT(4);
            __syncthreads();                                              // #2: reset flags out, this step's Philox words in
            QS_STAMP_AT(5);
            // the reset only computes: the terminal observation and state it overwrites wait in registers for the stores below
            float term_obs[12], term_sc[13];
            if (rs) {
#pragma unroll
                for (int i = 0; i < 12; ++i) term_obs[i] = obs[i];
#pragma unroll
                for (int i = 0; i < 13; ++i) term_sc[i] = sc[i];
                chaser_reset<PARAMS>(L, A, env, active, lane, t, sc, uc, ls, tt, P, obs);
            }
            QS_STAMP_AT(6);
            res_report_done(R, rep, seq + t + 1, tile, lane);             // the step's one memory wait (`rep`): before its stores
            if (rs) {
                if (D.term_obs && active) res_store_obs(D.term_obs, io, term_obs);
                res_store_term_half(D.term_state, active, io, 0, term_sc);
            }
            if (active) {
                res_store_obs(D.obs, o, obs);
                QS_SO(QS_GLOBAL_PTR(float, &D.reward[o]), reward);
                QS_SO(QS_GLOBAL_PTR(uint8_t, &D.done[o]), (uint8_t)(done ? 1 : 0));
                if (D.flags) QS_SO(QS_GLOBAL_PTR(uint8_t, &D.flags[o]), (uint8_t)flags);
            }
            D = Dn;
            cmd = cmdn;
        }
        if (t > 0) {
            if (active) {
                chaser_store(bw, sc, uc, ls, tt);
                if (PARAMS && RMODE == 2) store_par(A.par, tile, lane, P);
            }
        }
        {
            // the tile leaves: its step counter, its next descriptor, and -- after an EXIT -- its count towards the drain
            if (cmd != RES_SKIP && lane == 0) {
                if (t > 0) A.ctr[tile] = k0 + (uint64_t)t;
                R.rseq[tile] = seq + (unsigned long long)t + (cmd == RES_EXIT ? 1 : 0);
                if (cmd == RES_EXIT) {
                    const unsigned old = __hip_atomic_fetch_add(R.fin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (old + 1 == R.lane_tiles)
                        __hip_atomic_store(R.h_fin, seq + (unsigned long long)t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
#if defined(QS_STAMP) && QS_STAMP + 0 < 2
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        QS_STAMP_AT(7);
        QS_STAMP_FLUSH();
    } else if (role == 1) {
        float st[13], ut[4], qd[4];
        target_load(b, st, ut, qd);
#if defined(QS_STAMP) && QS_STAMP + 0 < 2
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        QS_STAMP_AT(1);
        int64_t t = 0;
#pragma clang loop unroll(disable)
        for (; cmd == RES_STEP; ++t) {
            QS_STAMP_STEP();
            float pre[13];
#pragma unroll
            for (int i = 0; i < 13; ++i) pre[i] = st[i];
            const bool lim_t = drone_advance<INTEG>(st, ut, P, A.C.dt);   // with the previous limited control
            uint4 w0, w1;
            target_publish(L, A, env, lane, k0 + (uint64_t)t, t, st, lim_t, w0, w1);
            QS_STAMP_AT(2);
            __syncthreads();                                              // #1
            QS_STAMP_AT(3);
            float *const term_state = (float *)s_tsp[t & 1];             // before #2 (see s_tsp)
            target_command(A.C, qd, pre, P.m, ut);
            QS_STAMP_AT(4);
            __syncthreads();                                              // #2
            QS_STAMP_AT(5);
            if (L.done[lane]) {
                res_store_term_half(term_state, active, io, 1, st);
                target_reset<PARAMS>(L, A, env, active, lane, w0, w1, st, ut, P);
            }
            cmd = s_cmd[(t + 1) & 1];
        }
        if (active && t > 0) target_store(bw, st, ut, qd);
        QS_STAMP_AT(6);
        QS_STAMP_FLUSH();
    } else if constexpr (split_prep(RMODE, PREP)) {
        int64_t t = 0;
#pragma clang loop unroll(disable)
        for (; cmd == RES_STEP; ++t) {
            uint4 w0, w1 = make_uint4(0, 0, 0, 0);
            random_init_words<RMODE == 2>(A.rc, STREAM_AUTORESET, A.gid0 + (uint64_t)env, k0 + (uint64_t)t + 1, w0, w1);
            __syncthreads();                                              // #1
            prep_publish<PARAMS>(L, A.rc, lane, w0, w1);
            __syncthreads();                                              // #2
            cmd = s_cmd[(t + 1) & 1];
        }
    }
}

template <int INTEG, bool PARAMS, int RMODE, int PREP>
__global__ __launch_bounds__(3 * kTile) void k_env_split(StepArgs A)
{
    __shared__ SplitLds<RMODE, PREP> L;
    const int lane = threadIdx.x & (kTile - 1);
    const int role = threadIdx.x >> 6;
    const int64_t tile = launch_tile(A, blockIdx.x);   // grid = the tiles of this launch's env group
    const int64_t env = tile * kTile + lane;
    bool active = env < A.n;                     // idle lanes of the tail tile compute on zeros and store nothing
    const int64_t io = env - A.io_env0;          // row of this env in the I/O arrays
    QS_ASSERT(tile < A.tile_end && (!active || (io >= 0 && io < A.io_n)));
    // private-queue launches: the tile's owning XCD is requested here and examined only after the first compute phase (below),
    // so that the check costs no memory latency; a misplaced workgroup computes on whatever it loaded and stores nothing
    const unsigned owner_xcc = chain_owner_request(A, tile);
    const uint64_t k0 = step_counter_begin_vmem(A, tile);
    QS_STAMP_DECL;
    QS_STAMP_AT(0);
    const float *b = A.st + tile * (int64_t)(kRecWords * kTile) + lane;
    float *bw = A.st + tile * (int64_t)(kRecWords * kTile) + lane;
    Par P = A.par_nom;
    if (PARAMS) P = load_par(A.par, tile, lane);
    if (role == 0) {
        // in a roll-out the chaser wave is the long pole of every step while target waves on the same SIMD run ahead with
        // speculative draws: give it the issue slots first (roll-out 2.28 -> 2.13 us/step; no help for a single step)
        if (A.T > 1) __builtin_amdgcn_s_setprio(3);
        float sc[13], uc[4], ls, tt;
        chaser_load(b, sc, uc, ls, tt);
        // the action is requested LAST: loads return in issue order, and the action -- fresh from the caller, the one
        // operand that is not cache-resident -- is not needed before the integration (which uses the PREVIOUS limited
        // control, quadrotor.py:126-144) is done; its miss latency hides under drone_advance
        float4 av_next = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (A.actions && active) av_next = reinterpret_cast<const float4 *>(A.actions)[io];
#if defined(QS_STAMP) && QS_STAMP + 0 < 2
        asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
#endif
        QS_STAMP_AT(1);
#pragma clang loop unroll(disable)
        for (int64_t t = 0; t < A.T; ++t) {
            const uint64_t k = k0 + (uint64_t)t;
            const int64_t o = t * A.io_n + io;
            tt += 1.0f;
            const bool lim_c = drone_advance<INTEG>(sc, uc, P, A.C.dt);   // Drone.step's integration: previous control only
            if (A.owner && chain_owner_mismatch(A, tile, lane, owner_xcc)) active = false;
            float a[4];
            if (A.actions) {
                const float4 av = av_next;
                if (t + 1 < A.T && active) av_next = reinterpret_cast<const float4 *>(A.actions)[o + A.io_n];
                a[0] = av.x; a[1] = av.y; a[2] = av.z; a[3] = av.w;
            } else {
                random_action(A.rc.seed, A.gid0 + (uint64_t)env, k, a);
            }
            float u_c[4];
            chaser_command(a, P.m, u_c);
            u_limit(u_c, P.m * kG, uc);                                   // ... and the hand-over of the new limited control
            QS_STAMP_AT(2);
            __syncthreads();                                              // #1: the target's new state is in LDS
            QS_STAMP_AT(3);
            if (A.T == 1) __builtin_amdgcn_s_setprio(3);                 // single step: from here on this wave is the long pole
            float obs[12], reward;
            unsigned flags;
            bool done;
            const bool rs = chaser_score(L, lane, sc, a, tt, ls, A.C, A.auto_reset, lim_c, obs, reward, flags, done);
            QS_STAMP_AT(4);
            __syncthreads();                                              // #2: reset flags out, this step's Philox words in
            QS_STAMP_AT(5);
            if (rs) {
                if (A.term_obs && active) store_obs(A.term_obs, io, obs);
                store_term_half(A.term_state, active, io, 0, sc);
                chaser_reset<PARAMS>(L, A, env, active, lane, t, sc, uc, ls, tt, P, obs);
            }
            QS_STAMP_AT(6);
            if (active) {
                if (A.slab) {
                    float2 *row = reinterpret_cast<float2 *>(A.slab + o * 14);
#pragma unroll
                    for (int i = 0; i < 6; ++i) row[i] = make_float2(obs[2 * i], obs[2 * i + 1]);
                    row[6] = make_float2(reward, done ? 1.0f : 0.0f);
                } else {
                    store_obs(A.obs, o, obs);
                    QS_SO(&A.reward[o], reward);
                    QS_SO(&A.done[o], (uint8_t)(done ? 1 : 0));
                }
                if (A.flags) QS_SO(&A.flags[o], (uint8_t)flags);
            }
        }
        if (active) {
            chaser_store(bw, sc, uc, ls, tt);
            if (PARAMS && RMODE == 2) store_par(A.par, tile, lane, P);
        }
        if (!A.owner || active || env >= A.n) step_counter_end(A, tile, lane, k0);   // a misplaced tile's counter stays put, too
#if defined(QS_STAMP) && QS_STAMP + 0 < 2
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        QS_STAMP_AT(7);
        QS_STAMP_FLUSH();
    } else if (role == 1) {
        float st[13], ut[4], qd[4];
        target_load(b, st, ut, qd);
        if (A.T == 1) __builtin_amdgcn_s_setprio(3);   // single step: the chaser wave waits at #1 for this wave's step + draw
#if defined(QS_STAMP) && QS_STAMP + 0 < 2
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        QS_STAMP_AT(1);
#pragma clang loop unroll(disable)
        for (int64_t t = 0; t < A.T; ++t) {
            float pre[13];
#pragma unroll
            for (int i = 0; i < 13; ++i) pre[i] = st[i];
            const bool lim_t = drone_advance<INTEG>(st, ut, P, A.C.dt);   // with the previous limited control
            if (A.owner && chain_owner_mismatch(A, tile, lane, owner_xcc)) active = false;
            uint4 w0, w1;
            target_publish(L, A, env, lane, k0 + (uint64_t)t, t, st, lim_t, w0, w1);
            QS_STAMP_AT(2);
            __syncthreads();                                              // #1
            QS_STAMP_AT(3);
            if (A.T == 1) __builtin_amdgcn_s_setprio(0);
            target_command(A.C, qd, pre, P.m, ut);
            QS_STAMP_AT(4);
            __syncthreads();                                              // #2
            QS_STAMP_AT(5);
            if (L.done[lane]) {
                store_term_half(A.term_state, active, io, 1, st);
                target_reset<PARAMS>(L, A, env, active, lane, w0, w1, st, ut, P);
            }
        }
        if (active) target_store(bw, st, ut, qd);
        QS_STAMP_AT(6);
        QS_STAMP_FLUSH();
    } else if constexpr (split_prep(RMODE, PREP)) {
#pragma clang loop unroll(disable)
        for (int64_t t = 0; t < A.T; ++t) {
            uint4 w0, w1 = make_uint4(0, 0, 0, 0);
            random_init_words<RMODE == 2>(A.rc, STREAM_AUTORESET, A.gid0 + (uint64_t)env, k0 + (uint64_t)t + 1, w0, w1);
            __syncthreads();                                              // #1
            prep_publish<PARAMS>(L, A.rc, lane, w0, w1);
            __syncthreads();                                              // #2
        }
    }
}

// hovering-v0 (HoveringEnv.step, hovering_env.py:47-78): T fused steps, one drone per lane.  Uses rows F_SC..
// (state) and F_UC.. (last limited control) of the tile; obs [T,N,13] = state after the step (or the stored
// ini_state after an auto-reset, hovering_env.py:80-82).
template <int INTEG, bool PARAMS>
__global__ __launch_bounds__(kBlock) void k_hover(StepArgs A)
{
    const int lane = threadIdx.x & (kTile - 1);
    const int64_t tile = A.tile0 + (int64_t)blockIdx.x * (kBlock / kTile) + (threadIdx.x >> 6);
    const int64_t env = tile * kTile + lane;
    if (tile >= A.tile_end || env >= A.n) return;
    const int64_t io = env - A.io_env0;
    QS_ASSERT(io >= 0 && io < A.io_n);
    const uint64_t k0 = step_counter_begin(A, tile);
    float *b = A.st + tile * (int64_t)(kRecWords * kTile) + lane;
    float s[13], up[4];
#pragma unroll
    for (int i = 0; i < 13; ++i) s[i] = b[(F_SC + i) * kTile];
#pragma unroll
    for (int i = 0; i < 4; ++i) up[i] = b[(F_UC + i) * kTile];
    Par P = A.par_nom;
    if (PARAMS) P = load_par(A.par, tile, lane);
#pragma clang loop unroll(disable)
    for (int64_t t = 0; t < A.T; ++t) {
        const int64_t o = t * A.io_n + io;
        float a[4];
        if (A.actions) {
            const float4 av = reinterpret_cast<const float4 *>(A.actions)[o];
            a[0] = av.x; a[1] = av.y; a[2] = av.z; a[3] = av.w;
        } else {
            random_action(A.rc.seed, A.gid0 + (uint64_t)env, k0 + (uint64_t)t, a);
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = 0.5f * a[i] + 0.5f;    // hovering actions live in [0,1]
        }
        float reward;
        unsigned flags;
        hover_step<INTEG>(s, up, a, P, A.C.dt, reward, flags);
        const bool done = (flags & FLAG_OVERLIMIT) != 0;
        if (done && A.auto_reset) {
            if (A.term_obs) for (int i = 0; i < 13; ++i) A.term_obs[io * 13 + i] = s[i];
            const float *src = A.init + env * 13;
#pragma unroll
            for (int i = 0; i < 13; ++i) s[i] = src[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) up[i] = 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 13; ++i) A.obs[o * 13 + i] = s[i];
        A.reward[o] = reward;
        A.done[o] = done ? 1 : 0;
        if (A.flags) A.flags[o] = (uint8_t)flags;
    }
#pragma unroll
    for (int i = 0; i < 13; ++i) b[(F_SC + i) * kTile] = s[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) b[(F_UC + i) * kTile] = up[i];
    step_counter_end(A, tile, lane, k0);
}

// construction-time jitter of docking-v1 (imitating_docking_env.py:34: chaser pos += U(-0.3,0.3)^3) and
// hovering-v0 (hovering_env.py:23-24: pos = (0,0,5)+U(-1,1)^3, att = euler2quat(U(-0.2,0.2)^3)), drawn from
// the rocRAND INIT stream (ctr 0) instead of numpy's global RNG; same 16-bit lattice as random_init.
__global__ __launch_bounds__(kBlock) void k_ctor_init(float *init, int64_t n, int hover, uint64_t seed, uint64_t gid0)
{
    const int64_t env = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (env >= n) return;
    uint4 w = philox_block(seed, STREAM_CTOR, gid0 + (uint64_t)env, 0);
    if (!hover) {
        float *d = init + env * 26;
        for (int i = 0; i < 26; ++i) d[i] = 0.0f;
        d[0] = __fmaf_rn(sym(u16lo(w.x)), 0.3f, 8.0f);
        d[1] = __fmaf_rn(sym(u16hi(w.x)), 0.3f, -50.0f);
        d[2] = __fmaf_rn(sym(u16lo(w.y)), 0.3f, 5.0f);
        d[6] = 1.0f;
        d[13] = 10.0f; d[14] = -50.0f; d[15] = 5.0f; d[19] = 1.0f;
    } else {
        float *d = init + env * 13;
        for (int i = 0; i < 13; ++i) d[i] = 0.0f;
        d[0] = sym(u16lo(w.x));
        d[1] = sym(u16hi(w.x));
        d[2] = __fmaf_rn(sym(u16lo(w.y)), 1.0f, 5.0f);
        float e0 = sym(u16hi(w.y)) * 0.2f, e1 = sym(u16lo(w.z)) * 0.2f, e2 = sym(u16hi(w.z)) * 0.2f;
        float sr, cr, sp, cp, sy, cy;
        q_sincos_small(0.5f * e0, sr, cr);
        q_sincos_small(0.5f * e1, sp, cp);
        q_sincos_small(0.5f * e2, sy, cy);
        euler2quat_trig(sr, cr, sp, cp, sy, cy, d + 6);
    }
}

__global__ __launch_bounds__(kBlock) void k_fill_init_nominal(float *init, int64_t n)
{
    const int64_t env = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (env >= n) return;
    float sc[13], st[13];
    nominal_init(sc, st);
    for (int i = 0; i < 13; ++i) { init[env * 26 + i] = sc[i]; init[env * 26 + 13 + i] = st[i]; }
}

// K2: masked reset (DockingEnv.reset, docking_env.py:233-244); init_all also rewrites q_des, like __init__
__global__ __launch_bounds__(kBlock) void k_reset(StepArgs A, const uint8_t *__restrict__ mask, int init_all)
{
    const int lane = threadIdx.x & (kTile - 1);
    const int64_t tile = (int64_t)blockIdx.x * (kBlock / kTile) + (threadIdx.x >> 6);
    const int64_t env = tile * kTile + lane;
    if (env >= A.n) return;
    if (mask && !mask[env]) return;
    Env e;
    load_env(A.st, tile, lane, e);
    float ic[13], it[13], obs[12];
    if (A.init) {
        const float *src = A.init + env * 26;
        for (int i = 0; i < 13; ++i) { ic[i] = src[i]; it[i] = src[13 + i]; }
    } else if (A.randomise) {
        Par Pn;
        random_init<true>(A.rc, STREAM_RESET, A.gid0 + (uint64_t)env, A.ctr[tile], ic, it, Pn);
        if (A.randomise >= 2) store_par(A.par, tile, lane, Pn);
    } else {
        nominal_init(ic, it);
    }
    if (init_all) { e.qd[0] = 1.0f; e.qd[1] = 0.0f; e.qd[2] = 0.0f; e.qd[3] = 0.0f; }
    env_reset(e, ic, it, obs);
    store_env(A.st, tile, lane, e);
    if (A.obs) store_obs(A.obs, env, obs);
}

// HoveringEnv.reset (hovering_env.py:80-82): state <- stored ini_state, last control <- 0; obs = the state
__global__ __launch_bounds__(kBlock) void k_hover_reset(StepArgs A, const uint8_t *__restrict__ mask)
{
    const int lane = threadIdx.x & (kTile - 1);
    const int64_t tile = (int64_t)blockIdx.x * (kBlock / kTile) + (threadIdx.x >> 6);
    const int64_t env = tile * kTile + lane;
    if (env >= A.n) return;
    if (mask && !mask[env]) return;
    float *b = A.st + tile * (int64_t)(kRecWords * kTile) + lane;
    const float *src = A.init + env * 13;
    for (int i = 0; i < 13; ++i) { b[(F_SC + i) * kTile] = src[i]; if (A.obs) A.obs[env * 13 + i] = src[i]; }
    for (int i = 0; i < 4; ++i) b[(F_UC + i) * kTile] = 0.0f;
}

__global__ __launch_bounds__(kBlock) void k_fill_ctr(unsigned long long *ctr, int64_t tiles, unsigned long long k)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < tiles) ctr[i] = k;
}

__global__ void k_nominal_obs(float *out)
{
    float sc[13], st[13], o[12];
    nominal_init(sc, st);
    rel_obs(sc, st, o);
    for (int i = 0; i < 12; ++i) out[i] = o[i];
}

__global__ __launch_bounds__(kBlock) void k_fill_par(float *par, int64_t n, Par P)
{
    const int lane = threadIdx.x & (kTile - 1);
    const int64_t tile = (int64_t)blockIdx.x * (kBlock / kTile) + (threadIdx.x >> 6);
    if (tile * kTile + lane >= n) return;
    store_par(par, tile, lane, P);
}

__global__ __launch_bounds__(kBlock) void k_fill_actions(float *__restrict__ actions, int64_t n, int64_t T, uint64_t seed,
                                                         uint64_t gid0, uint64_t step0)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n * T) return;
    const int64_t t = i / n, env = i - t * n;
    float a[4];
    random_action(seed, gid0 + (uint64_t)env, step0 + (uint64_t)t, a);
    reinterpret_cast<float4 *>(actions)[i] = make_float4(a[0], a[1], a[2], a[3]);
}

// AoS <-> AoSoA conversion for qs_get_state / qs_set_state / params
struct StateIO {
    float *chaser, *target, *u_prev, *qdes, *ls, *t;
};
template <bool TO_USER>
__global__ __launch_bounds__(kBlock) void k_state_io(float *st, int64_t n, StateIO io)
{
    const int lane = threadIdx.x & (kTile - 1);
    const int64_t tile = (int64_t)blockIdx.x * (kBlock / kTile) + (threadIdx.x >> 6);
    const int64_t env = tile * kTile + lane;
    if (env >= n) return;
    float *b = st + tile * (int64_t)(kRecWords * kTile) + lane;
    auto mv = [&](float *user, int f) {
        if (!user) return;
        if (TO_USER) *user = b[f * kTile];
        else b[f * kTile] = *user;
    };
    for (int i = 0; i < 13; ++i) mv(io.chaser ? io.chaser + env * 13 + i : nullptr, F_SC + i);
    for (int i = 0; i < 13; ++i) mv(io.target ? io.target + env * 13 + i : nullptr, F_ST + i);
    for (int i = 0; i < 8; ++i) mv(io.u_prev ? io.u_prev + env * 8 + i : nullptr, F_UC + i);
    for (int i = 0; i < 4; ++i) mv(io.qdes ? io.qdes + env * 4 + i : nullptr, F_QD + i);
    mv(io.ls ? io.ls + env : nullptr, F_LS);
    mv(io.t ? io.t + env : nullptr, F_T);
}

template <bool TO_USER>
__global__ __launch_bounds__(kBlock) void k_par_io(float *par, int64_t n, float *mass, float *inertia)
{
    const int lane = threadIdx.x & (kTile - 1);
    const int64_t tile = (int64_t)blockIdx.x * (kBlock / kTile) + (threadIdx.x >> 6);
    const int64_t env = tile * kTile + lane;
    if (env >= n) return;
    float *b = par + tile * (int64_t)(kParWords * kTile) + lane;
    if (TO_USER) {
        if (mass) mass[env] = b[0];
        if (inertia) for (int i = 0; i < 3; ++i) inertia[env * 3 + i] = b[(1 + i) * kTile];
    } else {
        if (mass) b[0] = mass[env];
        if (inertia) for (int i = 0; i < 3; ++i) b[(1 + i) * kTile] = inertia[env * 3 + i];
    }
}

inline int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }
inline unsigned grid_tiles(int64_t n) { return (unsigned)((tiles_of(n) + (kBlock / kTile) - 1) / (kBlock / kTile)); }
inline unsigned grid_flat(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace
