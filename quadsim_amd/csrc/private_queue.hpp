// private_queue.hpp -- the handle's private AQL queues (qs_set_queue_mode): step launches without the end-of-kernel release
// A fragment of quadsim_hip.hip (ONE translation unit: the kernels' mangled names, which the private-queue code resolves
// in the code object, live in that unit's anonymous namespace); included there at a fixed position, nowhere else.
#pragma once

// ---- private AQL queue for the step launches (qs_set_queue_mode) -------------------------------------------------------
// Every kernel HIP launches ends with an agent-scope release: the eight XCD L2s are not coherent with each other, so their
// dirty lines are written back before the next packet may start.  For a chain of dependent step launches that write-back is
// 1.6 of 6.5 us per step at 65 536 envs (profiles/r02/ab_experiments.txt, section E) -- and it is not needed: tile b is
// stepped by workgroup b of every launch, workgroup b always lands on the same XCD, so the tile's state can stay dirty in
// that XCD's L2 from one step to the next.  HIP has no launch without the fence; an AQL packet written by hand has:
//     header = KERNEL_DISPATCH | BARRIER (ordered behind the previous packet) | ACQUIRE agent (fresh kernargs / actions;
//              0.16 us, does not touch dirty lines) | RELEASE none.
// The handle therefore owns an HSA queue, loads its own copy of the library's code object into it, and writes one packet per
// qs_step.  Everything else stays on HIP: any other entry point first DRAINS the queue with a release packet (host wait).
//
// Ordering against the CALLER's work (the handle's stream S), round 3 -- QS_ORDER_STREAM, the default where the device has
// stream memory operations: a step behaves like a launch on S although it runs elsewhere.  Per submission (one qs_step, or the
// T steps of qs_rollout_stepwise):
//     S:      hipStreamWriteValue64(fwd, n)              -- executes when everything enqueued on S so far has finished
//     queue:  barrier-value packet (fwd >= n) | step packet(s), the last one with a completion signal `rev`
//     S:      hipStreamWaitValue64(rev == V0 - n)        -- whatever is enqueued on S afterwards runs after the step(s)
// and that last packet carries an agent-scope RELEASE, so that the outputs of all T steps are in memory -- not dirty in one XCD's
// L2 -- when `rev` fires (the state lines are written back with them and stay valid in their L2).  No host synchronisation
// anywhere.  A per-step loop (T = 1) thereby pays what a HIP launch pays -- per-step consumable outputs ARE the write-back:
// write-through output stores instead of the release were measured no faster (the kernel then ends when memory, not the L2,
// acknowledges its stores) -- plus the hand-shake; a T-step roll-out pays both once.  QS_ORDER_HOST is round 2's contract:
// inputs complete at the call, outputs valid after qs_sync (no hand-shake packets).
struct QsChainLane {                  // one private queue and the contiguous tile range it steps
    hsa_queue_t *queue = nullptr;
    char *kernargs = nullptr;
    std::vector<uint64_t> slot_qidx;  // queue index of the packet that last used each kernarg slot
    uint64_t issued = 0;              // step packets written so far
    int64_t tile0 = 0, tile_end = 0;
    hsa_signal_t done{};
    // QS_ORDER_STREAM: completion signal of this lane's submissions.  Allocated by HIP as "signal memory" (the only memory
    // hipStreamWaitValue64 accepts); HIP hands out the address of the signal's VALUE, the handle is the amd_signal_t around it.
    void *rev_ptr = nullptr;
    hsa_signal_t rev{};
    int64_t rev_value = 0;            // value of `rev` once every submission so far has completed (counts DOWN: AQL decrements)
    // resident roll-out (k_env_resident): this lane's dispatch
    char *res_kernarg = nullptr;      // its kernel-argument block (device memory, like the ring)
    hsa_signal_t res_done{};          // 1 while it runs, 0 once it has ended (its release included)
    bool res_launched = false;        // dispatched in the current roll-out (it may have ended since: idle limit)
    uint64_t res_prog = 0;            // the largest progress word seen from it (host view of ResArgs::h_prog)
};

// a kernel of the loaded code object, as an AQL dispatch packet needs it
struct QsKernel {
    uint64_t object = 0;
    uint32_t kernarg_size = 0, group_size = 0, private_size = 0;
    unsigned block = 0;
};

struct QsChain {
    hsa_agent_t gpu{}, cpu{};
    hsa_amd_memory_pool_t kernarg_pool{};
    std::vector<QsChainLane> lanes;
    int requested = 0;                // the queue count qs_set_queue_mode was called with (lanes.size() may be smaller)
    hsa_executable_t exe{};
    hsa_code_object_reader_t reader{};
    bool have_exe = false, have_reader = false;
    std::vector<char> image;          // the gfx950 code object (kept alive for the executable)
    uint64_t kernel_object = 0;
    int v_integ = -1, v_params = -1, v_rmode = -1, v_split = -1, v_prep = -1;   // the instantiation kernel_object belongs to
    uint32_t kernarg_size = 0, group_size = 0, private_size = 0;
    unsigned block = 0;
    size_t stride = 0, slots = 0;
    unsigned *d_owner = nullptr;      // [tiles] 32-bit words, agent-scope atomics only
    unsigned *d_err = nullptr;        // the placement guard's error word: pinned, coherent HOST memory (d_err = its device address) -- a
    volatile unsigned *h_err = nullptr;   // misplaced workgroup sets it with a system-scope atomic, and every later submission sees it
                                          // without a synchronisation: a stream-ordered loop that never drains still fails within a few steps
    bool kernargs_on_device = false;  // kernarg ring in BAR-mapped device memory (else: host memory, correct but slow)
    bool dirty = false;               // packets enqueued since the last drain
    bool hip_dirty = true;            // the handle did HIP-side work since the last packet
    // QS_ORDER_STREAM
    bool stream_ordered = false;
    void *fwd_ptr = nullptr;          // value word of the forward signal (HIP signal memory)
    hsa_signal_t fwd{};
    uint64_t fwd_seq = 0;             // submissions so far
    int dbg_shift = 0;                // one-shot: the next step packet runs with StepArgs::dbg_shift (placement-guard test)
    bool pkt_unreleased = false;      // step packets without a release fence since the last drain / release barrier
    // resident roll-out (host-ordered mode): see "resident roll-out" below
    bool res_enabled = false;         // QS_RESIDENT (read at qs_set_queue_mode) and a BAR-mapped device pool for the ring
    bool res_dbg_packets = false;     // qs_debug_chain_poison_owner armed: the steps go through the packet chain and its guard
    bool res_open = false;            // descriptors written since the last EXIT
    bool res_fits = false;            // the resolved resident instantiation fits the chip in one round
    QsKernel res_kernel;
    int rv_integ = -1, rv_params = -1, rv_rmode = -1, rv_prep = -1;
    int64_t res_wave_cap = 0;         // waves of k_env_resident the chip holds at once
    unsigned long long *ring = nullptr;   // [ring_slots][8] descriptors (k_env_resident), BAR-mapped device memory
    size_t ring_slots = 0;
    uint64_t res_issued = 1;          // sequence number of the next descriptor (tags: 0 is never a valid one)
    uint64_t res_retired = 1;         // every tile has consumed every descriptor below this one
    uint64_t res_seq0 = 0;            // first descriptor of the current roll-out
    uint64_t res_idle_ticks = 0;
    uint64_t res_dispatches = 0;      // resident dispatches issued (qs_debug_chain_resident)
    unsigned long long *d_rseq = nullptr; // [tiles] ResArgs::rseq
    unsigned *d_rcnt = nullptr;       // [lanes][32]: kResWinSlots window counters, then the EXIT count
    volatile unsigned long long *h_res = nullptr;   // pinned host words, [lanes][8]: progress, EXIT count reached
    unsigned long long *d_hres = nullptr;           // ... their device address
};

namespace {

#define HSA_TRY(expr)                                                                                   \
    do {                                                                                                \
        hsa_status_t s_ = (expr);                                                                       \
        if (s_ != HSA_STATUS_SUCCESS) {                                                                 \
            const char *m_ = nullptr;                                                                   \
            hsa_status_string(s_, &m_);                                                                 \
            return fail(QS_ERR_HIP, "%s failed: %s", #expr, m_ ? m_ : "unknown HSA status");           \
        }                                                                                               \
    } while (0)

constexpr int64_t kRevStart = (int64_t)1 << 40;
// resident roll-out (see "resident roll-out" below)
constexpr int kResIdleUs = 50;
constexpr size_t kResRingSlots = 256;   // power of two; kResWinSlots > slots / kResWin + 2
constexpr size_t kResKernargBytes = 4096;
constexpr double kResTimeoutS = 30.0;   // bound of every host wait of the resident path
static_assert((kResRingSlots & (kResRingSlots - 1)) == 0 && kResWinSlots > kResRingSlots / kResWin + 2, "ring / window sizes");

struct AgentPick {
    uint32_t want_bdf, want_domain;
    int want_index, seen;
    hsa_agent_t gpu, cpu;
    bool have_gpu, have_cpu;
};

hsa_status_t chain_agent_cb(hsa_agent_t a, void *data)
{
    AgentPick *p = (AgentPick *)data;
    hsa_device_type_t t;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (t == HSA_DEVICE_TYPE_CPU && !p->have_cpu) { p->cpu = a; p->have_cpu = true; }
    if (t == HSA_DEVICE_TYPE_GPU) {
        uint32_t bdf = 0, dom = 0;
        const bool ok = hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) == HSA_STATUS_SUCCESS &&
                        hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &dom) == HSA_STATUS_SUCCESS;
        // the agent must be THE device of the handle: matched by PCI domain + bus/device/function (BDFID = bus << 8 | device << 3 |
        // function); by ordinal only when HIP cannot name the device's PCI address
        if (p->want_bdf != 0xffffffffu ? (ok && bdf == p->want_bdf && dom == p->want_domain) : p->seen == p->want_index) {
            p->gpu = a;
            p->have_gpu = true;
        }
        ++p->seen;
    }
    return HSA_STATUS_SUCCESS;
}

// device-local memory the host may write through the PCIe BAR: where HIP itself keeps kernel arguments on this platform
// (kernargs in host memory would cost every workgroup a PCIe read: 44 us per step instead of 5)
struct DevPoolPick {
    hsa_agent_t cpu;
    hsa_amd_memory_pool_t pool;
    bool found;
};
hsa_status_t chain_device_pool_cb(hsa_amd_memory_pool_t pool, void *data)
{
    DevPoolPick *p = (DevPoolPick *)data;
    hsa_amd_segment_t seg;
    if (hsa_amd_memory_pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_SEGMENT, &seg) != HSA_STATUS_SUCCESS || seg != HSA_AMD_SEGMENT_GLOBAL)
        return HSA_STATUS_SUCCESS;
    uint32_t flags = 0;
    bool alloc = false;
    hsa_amd_memory_pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_GLOBAL_FLAGS, &flags);
    hsa_amd_memory_pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_RUNTIME_ALLOC_ALLOWED, &alloc);
    if (!alloc || !(flags & HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_COARSE_GRAINED)) return HSA_STATUS_SUCCESS;
    hsa_amd_memory_pool_access_t acc = HSA_AMD_MEMORY_POOL_ACCESS_NEVER_ALLOWED;
    hsa_amd_agent_memory_pool_get_info(p->cpu, pool, HSA_AMD_AGENT_MEMORY_POOL_INFO_ACCESS, &acc);
    if (acc == HSA_AMD_MEMORY_POOL_ACCESS_NEVER_ALLOWED) return HSA_STATUS_SUCCESS;
    p->pool = pool;
    p->found = true;
    return HSA_STATUS_INFO_BREAK;
}

hsa_status_t chain_kernarg_pool_cb(hsa_amd_memory_pool_t pool, void *data)
{
    hsa_amd_segment_t seg;
    if (hsa_amd_memory_pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_SEGMENT, &seg) != HSA_STATUS_SUCCESS || seg != HSA_AMD_SEGMENT_GLOBAL)
        return HSA_STATUS_SUCCESS;
    uint32_t flags = 0;
    hsa_amd_memory_pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_GLOBAL_FLAGS, &flags);
    if (flags & HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_KERNARG_INIT) { *(hsa_amd_memory_pool_t *)data = pool; return HSA_STATUS_INFO_BREAK; }
    return HSA_STATUS_SUCCESS;
}

// the gfx950 code object of THIS library: the .hip_fatbin section of the shared object the code runs from holds a clang
// offload bundle; its amdgcn entry is the ELF that HIP itself loads
int chain_read_code_object(std::vector<char> &out)
{
    Dl_info di;
    if (!dladdr((void *)&chain_read_code_object, &di) || !di.dli_fname) return fail(QS_ERR_HIP, "queue mode: cannot locate the library file");
    const int fd = open(di.dli_fname, O_RDONLY);
    if (fd < 0) return fail(QS_ERR_HIP, "queue mode: cannot open %s", di.dli_fname);
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); return fail(QS_ERR_HIP, "queue mode: fstat failed"); }
    const char *base = (const char *)mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (base == MAP_FAILED) return fail(QS_ERR_HIP, "queue mode: mmap failed");
    int rc = fail(QS_ERR_HIP, "queue mode: no gfx950 code object in %s", di.dli_fname);
    const Elf64_Ehdr *eh = (const Elf64_Ehdr *)base;
    const Elf64_Shdr *sh = (const Elf64_Shdr *)(base + eh->e_shoff);
    const char *names = base + sh[eh->e_shstrndx].sh_offset;
    for (int i = 0; i < eh->e_shnum; ++i) {
        if (strcmp(names + sh[i].sh_name, ".hip_fatbin") != 0) continue;
        const char *fb = base + sh[i].sh_offset;
        const char magic[] = "__CLANG_OFFLOAD_BUNDLE__";
        if (sh[i].sh_size < 32 || memcmp(fb, magic, 24) != 0) break;
        uint64_t n;
        memcpy(&n, fb + 24, 8);
        const char *q = fb + 32;
        for (uint64_t k = 0; k < n; ++k) {
            uint64_t off, size, tl;
            memcpy(&off, q, 8); memcpy(&size, q + 8, 8); memcpy(&tl, q + 16, 8);
            const char *triple = q + 24;
            q += 24 + tl;
            if (tl >= 6 && memmem(triple, tl, "amdgcn", 6) && memmem(triple, tl, "gfx950", 6) && off + size <= sh[i].sh_size) {
                out.assign(fb + off, fb + off + size);
                rc = QS_OK;
            }
        }
        break;
    }
    munmap((void *)base, (size_t)st.st_size);
    return rc;
}

void chain_close(QsEnv *e)
{
    QsChain *c = e->chain;
    if (!c) return;
    // nothing may be left waiting on a hand-shake value that will never come
    if (c->fwd.handle) hsa_signal_store_screlease(c->fwd, INT64_MAX);
    for (QsChainLane &L : c->lanes) {
        if (L.queue) hsa_queue_destroy(L.queue);
        if (L.kernargs) hsa_amd_memory_pool_free(L.kernargs);
        if (L.done.handle) hsa_signal_destroy(L.done);
        if (L.rev_ptr) (void)hipFree(L.rev_ptr);
        if (L.res_kernarg) hsa_amd_memory_pool_free(L.res_kernarg);
        if (L.res_done.handle) hsa_signal_destroy(L.res_done);
    }
    if (c->ring) hsa_amd_memory_pool_free(c->ring);
    if (c->d_rseq) (void)hipFree(c->d_rseq);
    if (c->d_rcnt) (void)hipFree(c->d_rcnt);
    if (c->h_res) (void)hipHostFree((void *)c->h_res);
    if (c->fwd_ptr) (void)hipFree(c->fwd_ptr);
    if (c->have_exe) hsa_executable_destroy(c->exe);
    if (c->have_reader) hsa_code_object_reader_destroy(c->reader);
    if (c->d_owner) (void)hipFree(c->d_owner);
    if (c->h_err) (void)hipHostFree((void *)c->h_err);
    delete c;
    e->chain = nullptr;
}

// the step-kernel instantiation launch_env_on would pick for the handle AS IT IS NOW (qs_set_params / qs_set_init_state after
// qs_set_queue_mode change it): (re-)resolved against the loaded executable whenever it differs from the one in use
int chain_resolve_kernel(QsEnv *e)
{
    QsChain *c = e->chain;
    int64_t lane_tiles = 0;
    for (const QsChainLane &L : c->lanes) lane_tiles = std::max<int64_t>(lane_tiles, L.tile_end - L.tile0);
    if (c->lanes.empty()) lane_tiles = e->tiles;          // chain_open resolves once before the lanes exist: re-resolved at the first step
    const StepVariant v = step_variant(e, lane_tiles);
    const int integ = v.integ, rmode = v.rmode, params = v.params;
    const int split = v.family == kFamSplit ? 1 : 0;
    const int prep = split ? v.prep : 0;
    if (c->kernel_object && integ == c->v_integ && rmode == c->v_rmode && params == c->v_params && split == c->v_split && prep == c->v_prep) return QS_OK;
    char sym[160];
    if (split) snprintf(sym, sizeof sym, "_ZN12_GLOBAL__N_111k_env_splitILi%dELb%dELi%dELi%dEEEvNS_8StepArgsE.kd", integ, params, rmode, prep);
    else snprintf(sym, sizeof sym, "_ZN12_GLOBAL__N_15k_envILi%dELb%dELi%dEEEvNS_8StepArgsE.kd", integ, params, rmode);
    hsa_executable_symbol_t ks;
    uint64_t ko = 0;
    uint32_t ka = 0, gs = 0, ps = 0;
    HSA_TRY(hsa_executable_get_symbol_by_name(c->exe, sym, &c->gpu, &ks));
    HSA_TRY(hsa_executable_symbol_get_info(ks, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &ko));
    HSA_TRY(hsa_executable_symbol_get_info(ks, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_SIZE, &ka));
    HSA_TRY(hsa_executable_symbol_get_info(ks, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE, &gs));
    HSA_TRY(hsa_executable_symbol_get_info(ks, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE, &ps));
    if (ka < sizeof(StepArgs)) return fail(QS_ERR_HIP, "qs_set_queue_mode: kernel argument block is %u B, StepArgs %zu B", ka, sizeof(StepArgs));
    if (c->stride && (((size_t)ka + 255) & ~size_t(255)) > c->stride)
        return fail(QS_ERR_HIP, "queue mode: kernel argument block of %s (%u B) exceeds the ring's slot size", sym, ka);
    c->kernel_object = ko; c->kernarg_size = ka; c->group_size = gs; c->private_size = ps;
    c->block = split ? split_waves(rmode, prep) * kTile : kBlock;
    c->v_integ = integ; c->v_rmode = rmode; c->v_params = params; c->v_split = split; c->v_prep = prep;
    return QS_OK;
}

// HIP "signal memory": an HSA signal created by HIP, of which it hands out the address of the value word.  The handle our
// own AQL packets need is the amd_signal_t around that word (amd_hsa_signal.h: value at offset 8, 64-byte aligned).
int chain_alloc_hip_signal(void **value_ptr, hsa_signal_t *handle, int64_t initial)
{
    HIP_TRY(hipExtMallocWithFlags(value_ptr, 8, hipMallocSignalMemory));
    const uintptr_t h = (uintptr_t)*value_ptr - offsetof(amd_signal_t, value);
    if (h & (AMD_SIGNAL_ALIGN_BYTES - 1)) return fail(QS_ERR_HIP, "queue mode: HIP signal memory is not the value word of an amd_signal_t");
    handle->handle = (uint64_t)h;
    if (((amd_signal_t *)h)->kind != AMD_SIGNAL_KIND_USER) return fail(QS_ERR_HIP, "queue mode: HIP signal memory is not a user signal");
    hsa_signal_store_screlease(*handle, initial);
    if (hsa_signal_load_scacquire(*handle) != initial) return fail(QS_ERR_HIP, "queue mode: HIP signal memory does not behave like an HSA signal");
    return QS_OK;
}

bool chain_can_stream_order(QsEnv *e)
{
    int can = 0;
    return hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, e->cfg.device) == hipSuccess && can != 0;
}

int chain_enable_stream_order(QsEnv *e)
{
    QsChain *c = e->chain;
    if (!c->fwd_ptr) {
        int r = chain_alloc_hip_signal(&c->fwd_ptr, &c->fwd, 0);
        if (r) return r;
        c->fwd_seq = 0;
    }
    for (QsChainLane &L : c->lanes) {
        if (L.rev_ptr) continue;
        int r = chain_alloc_hip_signal(&L.rev_ptr, &L.rev, kRevStart);
        if (r) return r;
        L.rev_value = kRevStart;
    }
    c->stream_ordered = true;
    return QS_OK;
}

int chain_open(QsEnv *e, int nq)
{
    if (e->cfg.kind == QS_KIND_HOVERING_V0) return fail(QS_ERR_INVALID, "qs_set_queue_mode: docking envs only");
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "qs_set_queue_mode: device buffers only");
    QsChain *c = new (std::nothrow) QsChain();
    if (!c) return fail(QS_ERR_NOMEM, "qs_set_queue_mode: out of host memory");
    e->chain = c;
    auto body = [&]() -> int {
        HSA_TRY(hsa_init());
        char bus[32] = "";
        AgentPick pick{0xffffffffu, 0, e->cfg.device, 0, {}, {}, false, false};
        unsigned dom = 0, b = 0, d = 0, f = 0;
        if (hipDeviceGetPCIBusId(bus, sizeof bus, e->cfg.device) == hipSuccess && sscanf(bus, "%x:%x:%x.%x", &dom, &b, &d, &f) == 4) {
            pick.want_bdf = (b << 8) | (d << 3) | f;
            pick.want_domain = dom;
        }
        HSA_TRY(hsa_iterate_agents(chain_agent_cb, &pick));
        if (!pick.have_gpu || !pick.have_cpu) return fail(QS_ERR_HIP, "qs_set_queue_mode: no HSA agent for device %d (%s)", e->cfg.device, bus);
        c->gpu = pick.gpu; c->cpu = pick.cpu;
        hsa_status_t ps = hsa_amd_agent_iterate_memory_pools(c->cpu, chain_kernarg_pool_cb, &c->kernarg_pool);
        if (ps != HSA_STATUS_INFO_BREAK) return fail(QS_ERR_HIP, "qs_set_queue_mode: no kernarg memory pool");
        int r = chain_read_code_object(c->image);
        if (r) return r;
        HSA_TRY(hsa_code_object_reader_create_from_memory(c->image.data(), c->image.size(), &c->reader));
        c->have_reader = true;
        HSA_TRY(hsa_executable_create_alt(HSA_PROFILE_FULL, HSA_DEFAULT_FLOAT_ROUNDING_MODE_DEFAULT, nullptr, &c->exe));
        c->have_exe = true;
        HSA_TRY(hsa_executable_load_agent_code_object(c->exe, c->gpu, c->reader, nullptr, nullptr));
        HSA_TRY(hsa_executable_freeze(c->exe, nullptr));
        r = chain_resolve_kernel(e);
        if (r) return r;
        c->stride = (((size_t)c->kernarg_size + 255) & ~size_t(255)) + 256;   // room for any instantiation's hidden arguments
        // a small ring: a slot is rewritten only after its packet ran, and recently used kernarg lines are still in the caches
        // (4 096 slots: 5.43 us per step, 256: 5.27, 64 and 16: 5.24, 4: host-bound; profiles/r02/ab_experiments.txt, section E)
        c->slots = getenv("QS_CHAIN_SLOTS") ? (size_t)atoi(getenv("QS_CHAIN_SLOTS")) : 64;
        if (c->slots < 2 || c->slots > 4096) c->slots = 64;
        DevPoolPick dp{c->cpu, {}, false};
        (void)hsa_amd_agent_iterate_memory_pools(c->gpu, chain_device_pool_cb, &dp);
        c->kernargs_on_device = dp.found;
        // nq queues, each stepping a contiguous range of tiles (whole multiples of 8 tiles where possible: one per XCD)
        std::vector<int64_t> cut{0};
        for (int q = 1; q <= nq; ++q) {
            int64_t t1 = q == nq ? e->tiles : ((e->tiles * q / nq) + 7) / 8 * 8;
            if (t1 > e->tiles) t1 = e->tiles;
            if (t1 > cut.back()) cut.push_back(t1);        // small handles: fewer, non-empty lanes
        }
        c->lanes.resize(cut.size() - 1);
        for (size_t q = 0; q + 1 < cut.size(); ++q) {
            QsChainLane &L = c->lanes[q];
            L.tile0 = cut[q]; L.tile_end = cut[q + 1];
            HSA_TRY(hsa_queue_create(c->gpu, 4096, HSA_QUEUE_TYPE_SINGLE, nullptr, nullptr, UINT32_MAX, UINT32_MAX, &L.queue));
            if (dp.found) {
                HSA_TRY(hsa_amd_memory_pool_allocate(dp.pool, c->stride * c->slots, 0, (void **)&L.kernargs));
                HSA_TRY(hsa_amd_agents_allow_access(1, &c->cpu, nullptr, L.kernargs));
            } else {
                HSA_TRY(hsa_amd_memory_pool_allocate(c->kernarg_pool, c->stride * c->slots, 0, (void **)&L.kernargs));
                HSA_TRY(hsa_amd_agents_allow_access(1, &c->gpu, nullptr, L.kernargs));
            }
            memset(L.kernargs, 0, c->stride * c->slots);   // the hidden arguments behind StepArgs are never read: zeros
            L.slot_qidx.assign(c->slots, 0);
            HSA_TRY(hsa_signal_create(0, 0, nullptr, &L.done));
        }
        HIP_TRY(hipMalloc((void **)&c->d_owner, (size_t)e->tiles * sizeof(unsigned)));
        HIP_TRY(hipHostMalloc((void **)&c->h_err, 64, hipHostMallocMapped | hipHostMallocCoherent));
        *c->h_err = 0;
        HIP_TRY(hipHostGetDevicePointer((void **)&c->d_err, (void *)c->h_err, 0));
        // resident roll-out: on unless QS_RESIDENT=0 (A/B runs); needs the ring in device memory the host can write
        const char *res = getenv("QS_RESIDENT");
        c->res_enabled = dp.found && !(res && res[0] == '0');
        if (c->res_enabled) {
            int cus = 0;
            HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->cfg.device));
            c->res_wave_cap = (int64_t)cus * 4 * 3;          // 3 waves per SIMD: every k_env_resident has <= 168 VGPRs
            const char *idle = getenv("QS_RESIDENT_IDLE_US");
            c->res_idle_ticks = (uint64_t)(idle ? std::max(1, atoi(idle)) : kResIdleUs) * 100;   // s_memrealtime: 100 MHz
            c->ring_slots = kResRingSlots;
            HSA_TRY(hsa_amd_memory_pool_allocate(dp.pool, c->ring_slots * kResWords * 8, 0, (void **)&c->ring));
            HSA_TRY(hsa_amd_agents_allow_access(1, &c->cpu, nullptr, c->ring));
            memset(c->ring, 0, c->ring_slots * kResWords * 8);     // tag 0 / sequence 0: never a valid descriptor
            for (QsChainLane &L : c->lanes) {
                HSA_TRY(hsa_amd_memory_pool_allocate(dp.pool, kResKernargBytes, 0, (void **)&L.res_kernarg));
                HSA_TRY(hsa_amd_agents_allow_access(1, &c->cpu, nullptr, L.res_kernarg));
                memset(L.res_kernarg, 0, kResKernargBytes);
                HSA_TRY(hsa_signal_create(0, 0, nullptr, &L.res_done));
            }
            HIP_TRY(hipMalloc((void **)&c->d_rseq, (size_t)e->tiles * sizeof(unsigned long long)));
            HIP_TRY(hipMalloc((void **)&c->d_rcnt, c->lanes.size() * 32 * sizeof(unsigned)));
            HIP_TRY(hipHostMalloc((void **)&c->h_res, c->lanes.size() * 64, hipHostMallocMapped | hipHostMallocCoherent));
            memset((void *)c->h_res, 0, c->lanes.size() * 64);
            HIP_TRY(hipHostGetDevicePointer((void **)&c->d_hres, (void *)c->h_res, 0));
        }
        // stream-ordered hand-shake: needs HIP's stream memory operations and its signal memory; without them the mode
        // stays host-ordered (round 2's contract)
        const char *ord = getenv("QS_CHAIN_ORDER");            // "host": start with round 2's contract (A/B runs)
        if (!(ord && ord[0] == 'h') && chain_can_stream_order(e)) {
            r = chain_enable_stream_order(e);
            if (r) return r;
        }
        return QS_OK;
    };
    int rc;
    try { rc = body(); }                                 // no C++ exception may cross the C ABI
    catch (...) { rc = fail(QS_ERR_NOMEM, "qs_set_queue_mode: out of host memory"); }
    if (rc != QS_OK) chain_close(e);
    return rc;
}

// one AQL packet behind everything enqueued before it on lane L (barrier bit): kind 0 the step kernel, 1 a barrier-AND packet
// (drain), 2 an AMD barrier-value packet that holds the lane until `wait_sig` >= wait_value (the caller's stream is ready),
// 3 the resident step kernel (c->res_kernel)
enum { PKT_STEP = 0, PKT_BARRIER = 1, PKT_WAIT_VALUE = 2, PKT_RESIDENT = 3 };
uint64_t chain_write_packet(QsChain *c, QsChainLane &L, int kind, const void *kernarg, unsigned grid, int acquire, int release,
                            hsa_signal_t completion, hsa_signal_t wait_sig = hsa_signal_t{0}, int64_t wait_value = 0)
{
    const uint64_t idx = hsa_queue_add_write_index_relaxed(L.queue, 1);
    while (idx - hsa_queue_load_read_index_scacquire(L.queue) >= L.queue->size) __builtin_ia32_pause();
    void *slot = (char *)L.queue->base_address + (idx & (L.queue->size - 1)) * 64;
    uint32_t word0;                                 // header (16 bits) + the 16 bits behind it, published by ONE 32-bit store
    const uint16_t fences = (1 << HSA_PACKET_HEADER_BARRIER) | (acquire << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) |
                            (release << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE);
    if (kind == PKT_BARRIER) {
        hsa_barrier_and_packet_t *p = (hsa_barrier_and_packet_t *)slot;
        memset((char *)p + 4, 0, 60);
        p->completion_signal = completion;
        word0 = (uint16_t)((HSA_PACKET_TYPE_BARRIER_AND << HSA_PACKET_HEADER_TYPE) | fences);
    } else if (kind == PKT_WAIT_VALUE) {
        hsa_amd_barrier_value_packet_t *p = (hsa_amd_barrier_value_packet_t *)slot;
        memset((char *)p + 4, 0, 60);
        p->signal = wait_sig;
        p->value = wait_value;
        p->mask = -1;
        p->cond = HSA_SIGNAL_CONDITION_GTE;
        p->completion_signal = completion;
        word0 = (uint16_t)((HSA_PACKET_TYPE_VENDOR_SPECIFIC << HSA_PACKET_HEADER_TYPE) | fences) |
                ((uint32_t)HSA_AMD_PACKET_TYPE_BARRIER_VALUE << 16);
    } else {
        hsa_kernel_dispatch_packet_t *p = (hsa_kernel_dispatch_packet_t *)slot;
        const bool res = kind == PKT_RESIDENT;
        p->workgroup_size_x = (uint16_t)(res ? c->res_kernel.block : c->block); p->workgroup_size_y = 1; p->workgroup_size_z = 1;
        p->reserved0 = 0;
        p->grid_size_x = grid; p->grid_size_y = 1; p->grid_size_z = 1;
        p->private_segment_size = res ? c->res_kernel.private_size : c->private_size;
        p->group_segment_size = res ? c->res_kernel.group_size : c->group_size;
        p->kernel_object = res ? c->res_kernel.object : c->kernel_object;
        p->kernarg_address = (void *)kernarg;
        p->reserved2 = 0;
        p->completion_signal = completion;
        word0 = (uint16_t)((HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) | fences) |
                ((uint32_t)(1 << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS) << 16);
    }
    __atomic_store_n((uint32_t *)slot, word0, __ATOMIC_RELEASE);
    hsa_signal_store_screlease(L.queue->doorbell_signal, (hsa_signal_value_t)idx);
    return idx;
}

// ---- resident roll-out (host-ordered mode) ---------------------------------------------------------------------------
// A pre-staged roll-out does not need a launch per step: no output is consumed before qs_sync, and tiles never exchange
// data.  So the first host-ordered qs_step after a drain dispatches k_env_resident once per lane over the lane's tiles, and
// every qs_step writes ONE 64-B descriptor (the step's I/O pointers, tagged with its sequence number; step_kernels.hpp) into a
// ring in BAR-mapped device memory.  The tiles keep their state in registers, poll the ring a step ahead and end on an EXIT
// descriptor, which every draining entry point appends before it waits for the dispatches (host wait, bounded).  The ring
// needs no read-back and no doorbell per step: a descriptor that lands late is polled for, never misread.
//   Back-pressure: a slot is rewritten only when every tile has consumed the descriptor it held (the lanes' progress words,
//   written by the last tile of each window, in pinned host memory).
//   Idle limit: a tile that sees no new descriptor for QS_RESIDENT_IDLE_US (default kResIdleUs) stores its state and its
//   position and ends; a dispatch whose tiles have all ended is dispatched again by the next qs_step (or the wait that needs
//   it), and its tiles resume where they stopped.  Co-residency is therefore never needed for progress, only for speed.
//   Coherence: the dispatch acquires and releases at system scope, so state, step counter and outputs are in memory when it
//   has ended, whichever XCD ran a workgroup: the resident path needs no owner words and no placement guard.
// QS_RESIDENT=0 (read at qs_set_queue_mode) keeps the packet chain (A/B runs).

double res_now()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// The resident loop's own choice of the reset-preparation variant where the packet chain takes the third wave (PREP 2) and
// nothing forces one (QS_RESET_PREP, qs_debug_set_reset_prep).  All tiles of the handle are on the chip at once for the whole
// roll-out; up to kResPrepMaxTiles of them (2.25 waves per SIMD with three waves per tile) the third wave still runs beside the
// other two, above that it takes issue slots from the chaser waves and two waves per tile are faster
// (profiles/step_phases: measured at 256, 512, 768 and 1 024 tiles).
constexpr int64_t kResPrepMaxTiles = 768;
int res_prep_for(const QsEnv *e, const QsChain *c)
{
    if (c->v_prep != 2 || prep_forced().load(std::memory_order_relaxed) == 2) return c->v_prep;
    return e->tiles <= kResPrepMaxTiles ? 2 : 0;
}

// the resident instantiation matching the packet chain's (chain_resolve_kernel first) but for its own PREP (res_prep_for);
// res_fits says whether it may be used
int res_resolve_kernel(QsEnv *e)
{
    QsChain *c = e->chain;
    if (!c->v_split) { c->res_fits = false; return QS_OK; }
    const int prep = res_prep_for(e, c);
    if (c->res_kernel.object && c->v_integ == c->rv_integ && c->v_params == c->rv_params && c->v_rmode == c->rv_rmode && prep == c->rv_prep)
        return QS_OK;
    char sym[200];
    snprintf(sym, sizeof sym, "_ZN12_GLOBAL__N_114k_env_residentILi%dELb%dELi%dELi%dEEEvNS_8StepArgsENS_7ResArgsE.kd", c->v_integ,
             c->v_params, c->v_rmode, prep);
    hsa_executable_symbol_t ks;
    QsKernel k;
    HSA_TRY(hsa_executable_get_symbol_by_name(c->exe, sym, &c->gpu, &ks));
    HSA_TRY(hsa_executable_symbol_get_info(ks, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &k.object));
    HSA_TRY(hsa_executable_symbol_get_info(ks, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_SIZE, &k.kernarg_size));
    HSA_TRY(hsa_executable_symbol_get_info(ks, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE, &k.group_size));
    HSA_TRY(hsa_executable_symbol_get_info(ks, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE, &k.private_size));
    if (k.kernarg_size > kResKernargBytes) return fail(QS_ERR_HIP, "queue mode: kernel argument block of %s is %u B", sym, k.kernarg_size);
    const int waves = split_waves(c->v_rmode, prep);
    k.block = (unsigned)(waves * kTile);
    c->res_kernel = k;
    c->rv_integ = c->v_integ; c->rv_params = c->v_params; c->rv_rmode = c->v_rmode; c->rv_prep = prep;
    // every workgroup of every lane resident at once (the chaser waves of late workgroups would otherwise wait for the first
    // round's idle limit); scratch would be a private segment per wave for the whole roll-out
    c->res_fits = k.private_size == 0 && e->tiles * waves <= c->res_wave_cap;
    return QS_OK;
}

bool res_running(const QsChainLane &L) { return L.res_launched && hsa_signal_load_relaxed(L.res_done) != 0; }

// dispatch lane L's resident kernel: every tile from seq0 (!= 0) or from where it stopped (0); tiles already at or past
// stop_seq end at once
int res_launch(QsEnv *e, QsChainLane &L, uint64_t seq0, uint64_t stop_seq)
{
    QsChain *c = e->chain;
    const size_t q = (size_t)(&L - c->lanes.data());
    StepArgs A = make_args(e);
    A.tile0 = L.tile0; A.tile_end = L.tile_end;
    A.T = 1;
    ResArgs R{};
    R.ring = c->ring;
    R.rseq = c->d_rseq;
    R.wcnt = c->d_rcnt + q * 32;
    R.fin = R.wcnt + kResWinSlots;
    R.h_prog = c->d_hres + q * 8;
    R.h_fin = R.h_prog + 1;
    R.seq0 = seq0;
    R.base = c->res_seq0;
    R.stop_seq = stop_seq;
    R.slots_mask = c->ring_slots - 1;
    R.idle_ticks = c->res_idle_ticks;
    R.lane_tiles = (unsigned)(L.tile_end - L.tile0);
    const size_t roff = (sizeof(StepArgs) + alignof(ResArgs) - 1) / alignof(ResArgs) * alignof(ResArgs);
    memcpy(L.res_kernarg, &A, sizeof A);
    memcpy(L.res_kernarg + roff, &R, sizeof R);
    __builtin_ia32_sfence();
    (void)*(volatile uint32_t *)(L.res_kernarg + roff + sizeof R - sizeof(uint32_t));   // landed before the doorbell
    hsa_signal_store_relaxed(L.res_done, 1);
    chain_write_packet(c, L, PKT_RESIDENT, L.res_kernarg, (unsigned)((L.tile_end - L.tile0) * c->res_kernel.block),
                       HSA_FENCE_SCOPE_SYSTEM, HSA_FENCE_SCOPE_SYSTEM, L.res_done);
    L.res_launched = true;
    ++c->res_dispatches;
    return QS_OK;
}

// the host's view of consumption: the smallest progress word over the lanes
void res_refresh(QsChain *c)
{
    uint64_t m = UINT64_MAX;
    for (size_t q = 0; q < c->lanes.size(); ++q) {
        QsChainLane &L = c->lanes[q];
        L.res_prog = std::max<uint64_t>(L.res_prog, c->h_res[q * 8]);   // window words may land out of order: keep the largest
        m = std::min<uint64_t>(m, L.res_prog);
    }
    c->res_retired = std::max<uint64_t>(c->res_retired, m);
}

// write descriptor s (cmd 0: a step with A's I/O pointers, 1: EXIT) once its slot is free (bounded wait)
int res_write(QsEnv *e, uint64_t s, int cmd, const StepArgs *A)
{
    QsChain *c = e->chain;
    if (c->res_retired + c->ring_slots <= s) {
        const double t_end = res_now() + kResTimeoutS;
        for (;;) {
            res_refresh(c);
            if (c->res_retired + c->ring_slots > s) break;
            for (QsChainLane &L : c->lanes)                 // a dispatch whose tiles reached the idle limit: resume it
                if (L.res_launched && !res_running(L)) { int r = res_launch(e, L, 0, UINT64_MAX); if (r) return r; }
            if (res_now() > t_end)
                return fail(QS_ERR_HIP, "queue mode: the resident step kernel consumed no descriptor for %.0f s (descriptor %llu, all "
                            "consumed below %llu, first lane's progress %llu, %llu dispatches)", kResTimeoutS, (unsigned long long)s,
                            (unsigned long long)c->res_retired, (unsigned long long)c->h_res[0], (unsigned long long)c->res_dispatches);
            __builtin_ia32_pause();
        }
    }
    const unsigned long long p[7] = {
        A ? (unsigned long long)A->actions : 0, A ? (unsigned long long)A->obs : 0, A ? (unsigned long long)A->reward : 0,
        A ? (unsigned long long)A->done : 0, A ? (unsigned long long)A->flags : 0, A ? (unsigned long long)A->term_obs : 0,
        A ? (unsigned long long)A->term_state : 0};
    for (int i = 0; i < 7; ++i)
        if (p[i] & ~kResPtrMask) return fail(QS_ERR_INVALID, "queue mode: a buffer address above 2^48");
    // eight aligned 8-byte stores, each word tagged (k_env_resident validates every word by itself: no order among them)
    const unsigned long long tag = (unsigned long long)(s & 0xffff) << 48;
    volatile unsigned long long *w = c->ring + (s & (c->ring_slots - 1)) * kResWords;
    for (int i = 0; i < 7; ++i) w[i] = p[i] | tag;
    w[7] = ((unsigned long long)cmd << 32) | (unsigned long long)(uint32_t)(s >> 16) | tag;
    __builtin_ia32_sfence();                       // out of the write-combining buffers: the GPU sees it without a doorbell
    return QS_OK;
}

// the resident roll-out in progress ends: EXIT, then every lane's dispatch has ended with every tile at the EXIT (bounded wait)
int res_finish(QsEnv *e)
{
    QsChain *c = e->chain;
    if (!c->res_open) return QS_OK;
    const uint64_t s = c->res_issued;
    int r = res_write(e, s, 1, nullptr);
    if (r) return r;
    c->res_issued = s + 1;
    const double t_end = res_now() + kResTimeoutS;
    for (;;) {
        bool all = true;
        for (size_t q = 0; q < c->lanes.size(); ++q) {
            QsChainLane &L = c->lanes[q];
            if (res_running(L)) { all = false; continue; }
            if (hsa_signal_load_scacquire(L.res_done) == 0 && c->h_res[q * 8 + 1] >= s + 1) continue;
            r = res_launch(e, L, 0, s + 1);          // tiles that stopped at the idle limit before the EXIT: to the EXIT
            if (r) return r;
            all = false;
        }
        if (all) break;
        if (res_now() > t_end)
            return fail(QS_ERR_HIP, "queue mode: the resident step kernel did not end within %.0f s of its EXIT descriptor", kResTimeoutS);
        __builtin_ia32_pause();
    }
    c->res_retired = s + 1;
    c->res_open = false;
    return QS_OK;
}

// one host-ordered step through the resident kernel
int res_step(QsEnv *e, const StepArgs &A)
{
    QsChain *c = e->chain;
    if (!c->res_open) {
        // a new roll-out: the handle's HIP-side work has finished and this roll-out's counters start from zero
        if (c->hip_dirty) HIP_TRY(hipMemsetAsync(c->d_owner, 0xff, (size_t)e->tiles * sizeof(unsigned), e->stream));
        HIP_TRY(hipMemsetAsync(c->d_rcnt, 0, c->lanes.size() * 32 * sizeof(unsigned), e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        c->hip_dirty = false;
        if (c->pkt_unreleased) {
            // step packets of this handle left tiles' state dirty in an XCD's L2: written back before any workgroup may load it
            for (QsChainLane &L : c->lanes)
                chain_write_packet(c, L, PKT_BARRIER, nullptr, 0, HSA_FENCE_SCOPE_NONE, HSA_FENCE_SCOPE_SYSTEM, hsa_signal_t{0});
            c->pkt_unreleased = false;
        }
        c->res_seq0 = c->res_issued;
        for (QsChainLane &L : c->lanes) L.res_launched = false;
        c->res_open = true;
    }
    const uint64_t s = c->res_issued;
    int r = res_write(e, s, 0, &A);
    if (r) return r;
    c->res_issued = s + 1;
    for (QsChainLane &L : c->lanes)
        if (!L.res_launched) { r = res_launch(e, L, c->res_seq0, UINT64_MAX); if (r) return r; }
        else if (!res_running(L)) { r = res_launch(e, L, 0, UINT64_MAX); if (r) return r; }
    return QS_OK;
}

// every packet has run and what it wrote is visible to the whole system (host wait); reports a misplaced tile
int chain_drain(QsEnv *e)
{
    QsChain *c = e->chain;
    if (!c) return QS_OK;
    int rr = res_finish(e);
    if (!c->dirty) return rr;
    for (QsChainLane &L : c->lanes) {
        hsa_signal_store_relaxed(L.done, 1);
        chain_write_packet(c, L, PKT_BARRIER, nullptr, 0, HSA_FENCE_SCOPE_NONE, HSA_FENCE_SCOPE_SYSTEM, L.done);
    }
    const double t_end = res_now() + kResTimeoutS;
    for (QsChainLane &L : c->lanes)
        while (hsa_signal_wait_scacquire(L.done, HSA_SIGNAL_CONDITION_LT, 1, 1000000, HSA_WAIT_STATE_ACTIVE) != 0)
            if (res_now() > t_end) return fail(QS_ERR_HIP, "queue mode: the private queue did not drain within %.0f s", kResTimeoutS);
    c->dirty = false;
    c->pkt_unreleased = false;
    if (*c->h_err) {
        *c->h_err = 0;
        return fail(QS_ERR_HIP, "queue mode: a workgroup ran on another XCD than the one holding its tile; the steps since the last "
                                "synchronisation are invalid (this placement is not promised by HIP: use qs_set_queue_mode(env, 0))");
    }
    return rr;
}

// T consecutive steps (T kernarg blocks: steps[t] differ in their I/O pointers only) on every lane, behind ONE hand-shake with
// the handle's stream when the chain is stream-ordered
int chain_submit(QsEnv *e, const StepArgs *steps, int64_t T)
{
    QsChain *c = e->chain;
    if (c->res_open) { int rf = res_finish(e); if (rf) return rf; }   // the packet chain continues where the resident kernel ended
    if (*c->h_err) {
        // a workgroup of an EARLIER step found its tile on another XCD (the word is host memory: no synchronisation needed to see
        // it).  Reported here as well as at the next drain, so that a loop of nothing but steps cannot run on unnoticed; the flag
        // stays set until a draining call has reported it and re-armed the handle.
        return fail(QS_ERR_HIP, "queue mode: a workgroup ran on another XCD than the one holding its tile; the steps since the last "
                                "synchronisation are invalid (call qs_sync, then continue or use qs_set_queue_mode(env, 0))");
    }
    int r = chain_resolve_kernel(e);               // qs_set_params / qs_set_init_state since the last step?
    if (r) return r;
    if (c->stream_ordered) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(e->stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
            return fail(QS_ERR_INVALID, "queue mode: a private-queue step cannot be captured into a hipGraph (use qs_set_queue_mode(env, 0))");
    }
    if (c->hip_dirty) {
        // HIP-side work of the handle (reset, set_state, ...) must have finished, and no tile has an owning XCD yet
        HIP_TRY(hipMemsetAsync(c->d_owner, 0xff, (size_t)e->tiles * sizeof(unsigned), e->stream));
        if (!c->stream_ordered) HIP_TRY(hipStreamSynchronize(e->stream));    // stream-ordered: the write-value below is behind it
        c->hip_dirty = false;
    }
    const size_t nl = c->lanes.size();
    if (c->stream_ordered) {
        ++c->fwd_seq;
        HIP_TRY(hipStreamWriteValue64(e->stream, c->fwd_ptr, c->fwd_seq, 0));
        for (QsChainLane &L : c->lanes)
            chain_write_packet(c, L, PKT_WAIT_VALUE, nullptr, 0, HSA_FENCE_SCOPE_NONE, HSA_FENCE_SCOPE_NONE, hsa_signal_t{0}, c->fwd,
                               (int64_t)c->fwd_seq);
    }
    for (int64_t t = 0; t < T; ++t) {
        StepArgs A = steps[t];
        A.owner = c->d_owner;
        A.err = c->d_err;
        A.dbg_shift = c->dbg_shift;
        c->dbg_shift = 0;
        // all lanes' kernarg blocks first, ONE read-back behind them, then the packets: the read-back is a PCIe round trip
        char *ka[8];
        size_t slot[8];
        for (size_t q = 0; q < nl; ++q) {
            QsChainLane &L = c->lanes[q];
            A.tile0 = L.tile0; A.tile_end = L.tile_end;
            // the slot about to be rewritten belongs to step `issued - slots`, queue packet p: that kernel has FINISHED once the
            // packet behind it has been taken off the queue (every packet carries the barrier bit): read index past p + 1
            slot[q] = L.issued % c->slots;
            if (L.issued >= c->slots)
                while (hsa_queue_load_read_index_scacquire(L.queue) < L.slot_qidx[slot[q]] + 2) __builtin_ia32_pause();
            ka[q] = L.kernargs + slot[q] * c->stride;
            memcpy(ka[q], &A, sizeof A);
        }
        if (c->kernargs_on_device) {
            // posted writes through the BAR: reading the last word back makes sure they have landed before a doorbell rings
            __builtin_ia32_sfence();
            (void)*(volatile uint32_t *)(ka[nl - 1] + sizeof A - sizeof(uint32_t));
        }
        const bool last = t + 1 == T;
        for (size_t q = 0; q < nl; ++q) {
            QsChainLane &L = c->lanes[q];
            const int64_t tiles = L.tile_end - L.tile0;
            const unsigned grid = c->v_split ? (unsigned)(tiles * c->block)
                                                        : (unsigned)(((tiles + kBlock / kTile - 1) / (kBlock / kTile)) * kBlock);
            // stream-ordered: the LAST packet of the submission publishes -- agent-scope release (the outputs of all T steps leave
            // the L2s; the state lines are written back too but stay valid where they are) and the completion signal the
            // caller's stream waits for.  (Write-through `sc1` output stores on every step instead of this release were built
            // and measured: 6.90 against 5.74 us per step in a 600-step roll-out, and they cost the ordinary launches 0.9 us
            // through the store code they displaced; profiles/r03/ab_experiments.txt section I.)
            const bool sig = c->stream_ordered && last;
            L.slot_qidx[slot[q]] = chain_write_packet(c, L, PKT_STEP, ka[q], grid, HSA_FENCE_SCOPE_AGENT,
                                                      sig ? HSA_FENCE_SCOPE_AGENT : HSA_FENCE_SCOPE_NONE, sig ? L.rev : hsa_signal_t{0});
            ++L.issued;
            if (sig) --L.rev_value;
        }
    }
    c->dirty = true;
    c->pkt_unreleased = true;
    if (c->stream_ordered)
        for (QsChainLane &L : c->lanes)
            HIP_TRY(hipStreamWaitValue64(e->stream, L.rev_ptr, (uint64_t)L.rev_value, hipStreamWaitValueEq, ~0ull));
    return QS_OK;
}

// one step: through the resident kernel where it applies (host-ordered, the role-split kernel, every tile on the chip at once,
// no placement-guard test armed), else one packet per lane.  (The instantiation cannot change inside a roll-out: every call
// that changes it drains first.)
int chain_resident_fits(QsEnv *e, bool *resident)
{
    QsChain *c = e->chain;
    *resident = false;
    if (c->res_enabled && !c->stream_ordered && !c->dbg_shift && !c->res_dbg_packets && !*c->h_err) {
        int r = chain_resolve_kernel(e);
        if (r) return r;
        r = res_resolve_kernel(e);
        if (r) return r;
        *resident = c->res_fits;
    }
    return QS_OK;
}

int chain_step(QsEnv *e, const StepArgs &A)
{
    bool resident = false;
    int r = chain_resident_fits(e, &resident);
    if (r) return r;
    if (resident) return res_step(e, A);
    return chain_submit(e, &A, 1);
}

// the instantiation chain_step takes next (qs_debug_step_variant)
int chain_step_variant(QsEnv *e, StepVariant *v)
{
    QsChain *c = e->chain;
    bool resident = false;
    int r = chain_resident_fits(e, &resident);
    if (r) return r;
    if (!resident && (r = chain_resolve_kernel(e))) return r;
    v->family = resident ? kFamResident : c->v_split ? kFamChainSplit : kFamChainSerial;
    v->integ = c->v_integ; v->params = c->v_params; v->rmode = c->v_rmode;
    v->prep = resident ? c->rv_prep : c->v_split ? c->v_prep : -1;
    return QS_OK;
}

}  // namespace
