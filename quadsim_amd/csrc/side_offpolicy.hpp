// side_offpolicy.hpp -- the host path the three *_update entry points of the off-policy trainers share (ddpg.hip, td3.hip, sac.hip):
// the checks they make in common, in the order each of them makes them, the table of the call's tensors with the overlap test,
// Adam's bias correction, the head of a kernel's StepArgs and the copy launches.  Host code on side_host.hpp, in an anonymous
// namespace as that is.  The messages are the ABI's: the C callers and the tests match on them.
#pragma once
#include "side_host.hpp"
#include "train_offpolicy.hpp"

namespace {

// the arguments no update does without, then the three struct sizes.  `q`: the prefix of the library's struct names
template <class Nets, class Replay, class Hyper>
int check_call(const Nets *nets, const Replay *replay, const void *indices, const Hyper *hp, const void *workspace, const void *stats,
               const char *q)
{
    if (!nets || !replay || !indices || !hp || !workspace || !stats)
        return fail(kErrInvalid, "nets, replay, indices, hp, workspace and stats must not be NULL");
    if (nets->struct_size != sizeof(Nets)) return fail(kErrInvalid, "%sNets.struct_size is %u, expected %zu", q, nets->struct_size, sizeof(Nets));
    if (replay->struct_size != sizeof(Replay))
        return fail(kErrInvalid, "%sReplay.struct_size is %u, expected %zu", q, replay->struct_size, sizeof(Replay));
    if (hp->struct_size != sizeof(Hyper)) return fail(kErrInvalid, "%sHyper.struct_size is %u, expected %zu", q, hp->struct_size, sizeof(Hyper));
    return kOk;
}

int check_extent(int batch, int max_batch, int steps, int max_steps, int64_t n, int64_t t0)
{
    if (batch < 1 || batch > max_batch) return fail(kErrInvalid, "batch must be in [1, %d], got %d", max_batch, batch);
    if (steps < 1 || steps > max_steps) return fail(kErrInvalid, "steps must be in [1, %d], got %d", max_steps, steps);
    if (n < 1 || n > 0x7fffffffll) return fail(kErrInvalid, "n must be in [1, 2^31), got %lld", (long long)n);
    return check_adam_t0(t0, steps, "steps");
}

int check_discount(double gamma, double tau)
{
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(kErrInvalid, "gamma must be in [0, 1], got %g", gamma);
    if (!(tau > 0.0 && tau <= 1.0)) return fail(kErrInvalid, "tau must be in (0, 1], got %g", tau);
    return kOk;
}

// the sweep for NULL and alignment over the replay, the call's own tensors and nets x 6 (nw nets with weights, nm of them with
// moments and, where asked for, gradients), then the size of the workspace.  `bad`: what the library found in its own arguments
template <class Replay>
int check_tensors(bool bad, const Replay *replay, const void *indices, const void *counts, const void *stats, const void *workspace,
                  uint64_t workspace_bytes, size_t need, float *const *w, int nw, float *const *m, float *const *v, int nm, float *const *grads)
{
    bad = bad || misaligned(replay->obs0) || misaligned(replay->act) || misaligned(replay->rew) || misaligned(replay->obs1) ||
          misaligned(replay->done) || misaligned(indices) || misaligned(counts) || misaligned(stats) || misaligned(workspace, 15) ||
          !replay->obs0 || !replay->act || !replay->rew || !replay->obs1 || !replay->done;
    for (int i = 0; i < 6 * nw; ++i) bad = bad || !w[i] || misaligned(w[i]);
    for (int i = 0; i < 6 * nm; ++i)
        bad = bad || !m[i] || misaligned(m[i]) || !v[i] || misaligned(v[i]) || (grads && (!grads[i] || misaligned(grads[i])));
    if (bad) return fail(kErrInvalid, "a tensor of the nets, of the replay or of the call is NULL or not aligned");
    if (workspace_bytes < need)
        return fail(kErrInvalid, "the workspace has %llu bytes, the call needs %zu", (unsigned long long)workspace_bytes, need);
    return kOk;
}

// the tensors of a call and where they lie in the workspace (the copy kernel's table, once for the way in and once for the way out),
// and everything the call writes, against each other.  EXTRA: the outputs that are no part of the table
template <class Copy, int EXTRA>
struct CallTable {
    static constexpr int kTensors = sizeof(Copy::t) / sizeof(float *);
    struct Range {
        uintptr_t lo, hi;
    };
    Copy in{}, out{};
    Range rs[kTensors + EXTRA];
    int nt = 0, nr = 0;

    void writes(const void *p, size_t bytes) { rs[nr++] = Range{(uintptr_t)p, (uintptr_t)p + bytes}; }
    void add(float *p, int at, int n)
    {
        in.t[nt] = out.t[nt] = p;
        in.at[nt] = out.at[nt] = at;
        in.n[nt] = out.n[nt] = n;
        ++nt;
        writes(p, 4 * (size_t)n);
    }
    // the six tensors of a net of flat layout F that lies at `at`
    template <class F>
    void add_net(float *const *six, int at)
    {
        for (int i = 0; i < 6; ++i) add(six[i], at + F::at(i), F::elems(i));
    }
    int check_overlap() const
    {
        for (int a = 0; a < nr; ++a)
            for (int b = a + 1; b < nr; ++b)
                if (rs[a].lo < rs[b].hi && rs[b].lo < rs[a].hi) return fail(kErrInvalid, "two tensors the call writes overlap");
        return kOk;
    }
};

// the first n tensors of a table into the workspace (to_ws) or out of it
template <class Kernel, class Copy>
int launch_copy(Kernel kernel, Copy &C, int n, float *ws, int to_ws, hipStream_t st)
{
    C.ws = ws;
    C.to_ws = to_ws;
    hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(qsf::kCopyBlock), 0, st, C);
    HIP_TRY(hipGetLastError());
    return kOk;
}

// Adam's bias correction of step tt (from 1) on the learning rate
template <class Hyper>
double adam_corr(const Hyper *hp, double tt)
{
    return sqrt(1.0 - pow(hp->beta2, tt)) / (1.0 - pow(hp->beta1, tt));
}

// what the StepArgs of the three step kernels share and no step changes: the workspace, the replay, Adam's constants, the discount
// and the Polyak rate
template <class Args, class Replay, class Hyper>
void fill_step_head(Args &S, float *ws, const Replay *replay, const Hyper *hp, int batch)
{
    S.ws = ws;
    S.obs0 = replay->obs0; S.act = replay->act; S.rew = replay->rew; S.obs1 = replay->obs1; S.done = replay->done;
    S.b1f = (float)hp->beta1; S.b2f = (float)hp->beta2; S.omb1 = (float)(1.0 - hp->beta1); S.omb2 = (float)(1.0 - hp->beta2);
    S.eps = (float)hp->eps;
    S.gamma = (float)hp->gamma; S.tau = (float)hp->tau; S.omt = (float)(1.0 - hp->tau);
    S.batch = batch;
}

}  // namespace
