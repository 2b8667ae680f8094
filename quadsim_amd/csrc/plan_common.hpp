// plan_common.hpp -- what the planner kernels of shooting.hpp, mppi.hpp, shooting_split.hpp and mppi_split.hpp share WITHOUT a
// change of their machine code (profiles/plan_host/README.md has the comparison): the position term of the score and a part's
// range of candidates.  The per-env prologue as a function moved k_mppi and is not here.  Nothing around env_step_target or
// env_step_chaser either: a function shared there moved the code of every planner kernel (profiles/plan_common/README.md), so
// the target-row loop and the candidate loop stay in the kernels.  A fragment of quadsim_hip.hip, included right before
// shooting.hpp, nowhere else.
#pragma once

namespace {

// the POSITION objective's term of one observation: -|rel_pos|^2
__device__ __forceinline__ float plan_pos(const float *obs) { return -(obs[0] * obs[0] + obs[1] * obs[1] + obs[2] * obs[2]); }

// part `part` of `splits` owns the candidates [lo, hi) = [part * ceil(paths / splits), + ceil(paths / splits)) cut at `paths`;
// trailing parts may be short or empty.  splits <= 1024, the chunk <= 65536: part * chunk fits an int
struct PlanPart { int lo, hi; };
__device__ __forceinline__ PlanPart plan_part(int part, int splits, int paths)
{
    const int chunk = (paths + splits - 1) / splits;
    const int lo = min(part * chunk, paths);
    return PlanPart{lo, min(lo + chunk, paths)};
}

}  // namespace
