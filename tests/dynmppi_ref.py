"""Float64 reference of MPPI over the learned dynamics net (qsdm_mppi_plan, include/quadsim_dyn_mppi.h): glue and nothing else.
The candidates and the update are tests/mppi_ref.py's (candidates32, update64), the model and the score tests/dynplan_ref.py's
(rollout64, cost64).  A helper module, not a test; numpy only."""
import numpy as np

import dynplan_ref as dr
import mppi_ref


def shifted(nominal, horizon, shift, n=None):
    """U of iteration 0: nominal[:, min(h + shift, horizon - 1)], zeros [n,horizon,4] without a nominal"""
    if nominal is None:
        return np.zeros((n, horizon, 4), np.float32)
    nominal = np.asarray(nominal, np.float32)
    return nominal[:, np.minimum(np.arange(horizon) + int(shift), horizon - 1)]


def iteration64(W, obs, U, sigma, z, lam):
    """one iteration from the float32 nominal U [N,horizon,4] and the noise z [paths,horizon,4] -> (the new nominal in float64,
    not rounded; the float64 scores [N,paths]; the float32 candidates [N,paths,horizon,4])"""
    cands = mppi_ref.candidates32(U, sigma, z)
    scores = dr.cost64(dr.rollout64(W, obs, cands))
    return mppi_ref.update64(scores, cands, lam, U), scores, cands


def plan64(W, obs, sigma, noise, lam, nominal=None, shift=0):
    """the whole plan with caller noise [iterations,paths,horizon,4]: the nominal is rounded to float32 between iterations, as
    the device keeps it -> dict(trace [N,iterations+1,horizon,4] float32, scores [N,iterations,paths], candidates (of the last
    iteration), nominal, actions, best_score)"""
    noise = np.asarray(noise, np.float32)
    iterations, paths, horizon = noise.shape[:3]
    obs = np.asarray(obs, np.float32)
    U = shifted(nominal, horizon, shift, len(obs))
    trace, scores, cands = [U], [], None
    for it in range(iterations):
        new, S, cands = iteration64(W, obs, U, sigma, noise[it], lam)
        U = new.astype(np.float32)
        trace.append(U)
        scores.append(S)
    S = scores[-1]
    with np.errstate(invalid="ignore"):
        best = np.max(np.where(np.isnan(S), -np.inf, S), axis=1)
    return dict(trace=np.stack(trace, axis=1), scores=np.stack(scores, axis=1), candidates=cands, nominal=U, actions=U[:, 0],
                best_score=best)
