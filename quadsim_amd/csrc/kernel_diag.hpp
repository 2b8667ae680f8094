// kernel_diag.hpp -- macros the kernels are written with: the in-kernel time stamps of the diagnostic builds (QS_STAMP_*,
// QS_PHASE_*; empty in the product build), the store flavour of the step kernels (QS_ST, QS_SO) and, for the resident step
// kernel, global-addressed pointers and the vmcnt wait (QS_GLOBAL_PTR, QS_WAIT_VMEM)
// A fragment of quadsim_hip.hip (ONE translation unit), included there right before step_kernels.hpp, nowhere else.
#pragma once

// -DQS_STAMP (diagnostic build, tools/build_stamp.sh): every workgroup of the role-split step kernel records the
// 100 MHz real-time counter at its phase boundaries into a caller-provided buffer (qs_debug_set_stamps), keyed by
// (step counter, tile) -- the in-kernel timeline of consecutive launches of the real chain.  Never in the product build.
#ifdef QS_STAMP
// The stamp buffer travels in StepArgs (not in a __device__ global): the private-queue launches run a second copy of the code
// object, loaded through HSA, whose globals HIP's hipMemcpyToSymbol never reaches.
// stamps stay in registers until the wave's last instruction: a store next to a barrier would be waited for by it
#define QS_STAMP_DECL unsigned long long stamp_[8] = {0, 0, 0, 0, 0, 0, 0, 0}; (void)stamp_
// -DQS_STAMP=2 ("light"): only the first and the last stamp of a wave.  The first stays in a register; the last -- taken when
// all of the wave's stores have been ISSUED, not drained -- is stored together with it by lane 0 (two 8-byte stores, never waited
// for).  The full build's eight scalar-memory round trips, its load-landed waits and, above all, its flush of eight stores
// BEHIND the drained wave end (a store-acknowledge latency on every workgroup's tail) cost ~0.7-0.9 us per step: too much for a
// timeline whose PERIOD is to be compared with the unstamped chain.  Even two stamps per wave cost ~0.4 us per step when every
// workgroup takes them (each is a scalar-memory round trip at the wave's head / tail), so only one workgroup in 64 does.
#if QS_STAMP + 0 >= 2
#define QS_STAMP_AT(slot)                                                                                       \
    do {                                                                                                        \
        /* no control flow near the loads: the first stamp is taken unconditionally (a scalar-memory read nobody waits */ \
        /* for until the wave's end); a branch here changes where the compiler waits for the state rows (+0.8 us)       */ \
        /* ... and it is taken at stamp site 1, BEHIND the issue of the wave's state loads (~50 ns after the wave's start): a  */ \
        /* scalar-memory read in front of them delays every later s_waitcnt lgkmcnt(0), i.e. the loads' addresses              */ \
        if ((slot) == 1) stamp_[0] = __builtin_amdgcn_s_memrealtime();                                          \
        else if ((slot) == (role == 0 ? 7 : 6)) {                                                               \
            if (lane == 0 && A.stamps && (tile & 63) == 0) {     /* one workgroup in 64 records */               \
                const unsigned long long now_ = __builtin_amdgcn_s_memrealtime();                               \
                const unsigned long long ix_ = ((k0 % 64ull) * (unsigned long long)(A.stamp_tiles) + (unsigned long long)tile) * 16ull + 8 * role; \
                if (ix_ + 8 <= A.stamp_cap) { A.stamps[ix_] = stamp_[0]; A.stamps[ix_ + (slot)] = now_; }       \
            }                                                                                                   \
        }                                                                                                       \
    } while (0)
#else
#define QS_STAMP_AT(slot) (stamp_[slot] = __builtin_amdgcn_s_memrealtime())
#endif
#if QS_STAMP + 0 >= 2
#define QS_STAMP_FLUSH() ((void)0)
#else
#define QS_STAMP_FLUSH()                                                                                        \
    do {                                                                                                        \
        if (lane == 0 && A.stamps) {                                                                            \
            const unsigned long long ix_ = ((k0 % 64ull) * (unsigned long long)(A.stamp_tiles) + (unsigned long long)tile) * 16ull + 8 * role; \
            if (ix_ + 8 <= A.stamp_cap) for (int j_ = 0; j_ < 8; ++j_) A.stamps[ix_ + j_] = stamp_[j_];          \
        }                                                                                                       \
    } while (0)
#endif
// runner kernels: phase durations summed over the T steps of one launch, [tile][role][8] words
#define QS_PHASE_DECL unsigned long long ph_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ph_t_ = __builtin_amdgcn_s_memrealtime(); \
    const unsigned long long ph_c0_ = __builtin_amdgcn_s_memtime(), ph_r0_ = ph_t_
#define QS_PHASE(slot) do { const unsigned long long n_ = __builtin_amdgcn_s_memrealtime(); ph_[slot] += n_ - ph_t_; ph_t_ = n_; } while (0)
#define QS_PHASE_FLUSH(role_)                                                                                   \
    do {                                                                                                        \
        ph_[6] = __builtin_amdgcn_s_memtime() - ph_c0_;          /* shader clocks ... */                         \
        ph_[7] = __builtin_amdgcn_s_memrealtime() - ph_r0_;      /* ... per 10 ns ticks = the clock frequency */ \
        if (lane == 0 && A.stamps) {                                                                            \
            const unsigned long long ix_ = (unsigned long long)tile * 16ull + 8 * (role_);                      \
            if (ix_ + 8 <= A.stamp_cap) for (int j_ = 0; j_ < 8; ++j_) A.stamps[ix_ + j_] = ph_[j_];             \
        }                                                                                                       \
    } while (0)
#else
#define QS_STAMP_DECL ((void)0)
#define QS_STAMP_AT(slot) ((void)0)
#define QS_STAMP_FLUSH() ((void)0)
#define QS_PHASE_DECL ((void)0)
#define QS_PHASE(slot) ((void)0)
#define QS_PHASE_FLUSH(role_) ((void)0)
#endif

// Store flavour of the step kernels' state rows and outputs: non-temporal (`nt`).  Every byte a step writes is consumed by a
// LATER launch (the next step, the policy), never by this one, and each launch ends with the write-back of the L2s' dirty lines:
// streaming stores leave that write-back less to do (65 536 envs: 6.92 -> 6.60 us per step; 131 072: 9.21 -> 8.87 us; plain
// stores with -DQS_PLAIN_STORES for A/B).  `sc1` write-through stores, in contrast, evict the lines and cost more than they save.
#if defined(QS_PLAIN_STORES)
#define QS_ST(p, v) (*(p) = (v))
#define QS_SO(p, v) QS_ST(p, v)
#else
#define QS_ST(p, v) __builtin_nontemporal_store((v), (p))
#define QS_SO(p, v) QS_ST(p, v)
#endif

// A pointer the compiler cannot trace to a kernel argument (the resident kernel rebuilds its I/O pointers from descriptor words)
// is a flat pointer: its stores count in lgkmcnt as well as vmcnt, so every LDS wait also waits for them.  The I/O arrays are
// device memory: a store through QS_GLOBAL_PTR is a global_store_* that only vmcnt tracks.
#define QS_GLOBAL __attribute__((address_space(1)))
#define QS_GLOBAL_PTR(T, p) ((QS_GLOBAL T *)(p))
// `s_waitcnt vmcnt(0)` as the builtin (gfx9 encoding: expcnt and lgkmcnt left at their maxima), which the compiler's own wait
// insertion takes into account; the asm waits of the stamp builds are invisible to it
#define QS_WAIT_VMEM() __builtin_amdgcn_s_waitcnt(0x0f70)
