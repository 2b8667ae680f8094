"""What the planners' rate tools share (shooting_rate.py, mppi_rate.py, shooting_split_rate.py, mppi_split_rate.py): the
handle they plan on, timed windows, rounds in which the configurations alternate, ranges over rounds, the single-env host path
and the --out file.  Every figure is per round; summaries are [min, max] ranges, never means."""
import json
import os
import time


def stepped_env(qa, n):
    """n docking-v0 envs with rocRAND initial states after a reset and two random steps"""
    env = qa.VecDockingEnv("docking-v0", num_envs=n, randomise=1, seed=5, init_range=qa.C3_INIT_RANGE)
    env.reset()
    for a in env.random_actions(2, step0=0):
        env.step(a)
    return env


def window(env, fn, reps):
    """`reps` calls of fn between qs_timer_start / qs_timer_stop on the handle's stream -> (stream ms per call, fn's last result)"""
    env.timer_start()
    for _ in range(reps):
        r = fn()
    return env.timer_stop() / reps, r


def alternating_rounds(torch, env, configs, plan, rounds, reps, cell):
    """Rounds 1 .. `rounds` after round 0, which warms up and is not reported: in every round each (name, s) of `configs` gets
    one window of `reps` calls of plan(s), in the order of `configs` in odd rounds and reversed in even ones -> one row per
    round with the keys of `cell`, NAME_ms (stream time per call, which includes the gap in which the host reads the step
    counter back and launches) and NAME_wall_ms (wall time per call).  Each row is printed as a JSON line."""
    rows = []
    for rnd in range(rounds + 1):
        row = dict(cell, round=rnd)
        for name, s in (configs if rnd % 2 else configs[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            row[name + "_ms"], _ = window(env, lambda: plan(s), reps)
            row[name + "_wall_ms"] = (time.perf_counter() - t0) * 1e3 / reps
        if rnd:
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def ranges(rows, keys):
    """{key: [min, max] over the rows}"""
    return {k: [min(r[k] for r in rows), max(r[k] for r in rows)] for k in keys}


def ratio_range(rows, num, den):
    return [min(r[num] / r[den] for r in rows), max(r[num] / r[den] for r in rows)]


def host_path(qa, rounds, plan_and_step, iters=200, **cell):
    """Wall time per plan + step iteration of the single-env shim, per round after a warm-up round.  plan_and_step(env, carry)
    plans, adds the plan's wall time to carry["plan_s"] and steps; `carry` starts empty in every round."""
    env = qa.DockingEnv()
    rows = []
    for rnd in range(rounds + 1):
        env.reset()
        carry = dict(plan_s=0.0)
        t0 = time.perf_counter()
        for _ in range(iters):
            plan_and_step(env, carry)
        dt = time.perf_counter() - t0
        if rnd:
            rows.append(dict(round=rnd, iterations=iters, plan_and_step_ms=dt / iters * 1e3, plan_ms=carry["plan_s"] / iters * 1e3))
    splits = qa.plan_splits(env, 200)
    env.close()
    return dict(cell, auto_splits=splits, control_period_ms=20.0, rounds=rows, **ranges(rows, ("plan_and_step_ms", "plan_ms")))


def write_out(path, torch, **fields):
    """the --out file: device, date, then `fields` in their order; one line per top-level key, and per element of a list"""
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    doc = dict(device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"), **fields)
    line = lambda v: ("[\n  " + ",\n  ".join(json.dumps(x) for x in v) + "\n ]") if isinstance(v, list) and v else json.dumps(v)   # noqa: E731
    with open(path, "w") as f:
        f.write("{\n " + ",\n ".join("%s: %s" % (json.dumps(k), line(v)) for k, v in doc.items()) + "\n}\n")
