"""What scoring a tree of arc segments on the grid's plan costs (kicp_grid_score_arc_tree), one process, the caller bound as
tools/bench_pipeline.py binds it.

Scene and plan: tools/bench_arcs.py's - the grid left by a short drive in cfg1's scene at 0.05 m cells with kicp_grid_potential's plan
in the handle, and the OPEN FLOOR, a second handle of the same geometry over a costmap of zeros, where nothing collides before it
leaves the grid.  The same 1.0 x 0.6 m box sampled at 0.05 m (21 x 13 samples), dt = 0.1 s, from the pose the robot stands at.
The trees: branch (16, 8, 8) and (8, 8, 8, 8), 8 steps a level.  A level's primitives are a lattice of commands, v up to 1.5 m/s and
omega across +-1.5 rad/s (4 x 4 for 16, 2 x 4 for 8).  Per tree and floor, the host clock around the call:
  - kicp_grid_score_arc_tree: one launch per level on the plan where it lies in HBM; returns after the N x 4 words have arrived;
  - kicp_score_arc_tree_from_plan: the same arithmetic on the host, one thread - its values are checked against the device's;
  - kicp_grid_score_arcs on the same plan with as many arcs as the tree has leaves (a v x omega lattice of n_D commands) and as many
    steps as a path has: the flat fan's kernel on as many leaves and steps - the comparison.  Its arcs are other trajectories than the
    tree's paths, so beside each time stands the number of poses the call checked, read off its results.
By operation count a tree checks at most sum n_d L_d poses where n_D sequences rolled from the start check n_D T.
Every entry writes into an array allocated once (`out=`).  Warm; the calls alternate `rounds` times; median, p10 / p90, min .. max.
On the open floor the host entry is timed in 5 of the rounds only.  Prints one JSON line.

    python tools/bench_arc_tree.py [--rounds 30] [--frames 8]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kinematic_icp_amd as K  # noqa: E402
from bench_arcs import BOX, DT  # noqa: E402
from bench_clearance import cases  # noqa: E402
from bench_grid import make_grid  # noqa: E402
from bench_pipeline import placement  # noqa: E402
from bench_potential import KW, plan  # noqa: E402
from bench_relocalize import spread  # noqa: E402

TREES = ((16, 8, 8), (8, 8, 8, 8))
LEVEL_STEPS = 8
LATTICE = {16: (4, 4), 8: (2, 4)}  # v x omega of a level's primitives


def level_commands(b):
    nv, nw = LATTICE[b]
    v, omega = np.meshgrid(np.linspace(1.5 / nv, 1.5, nv), np.linspace(-1.5, 1.5, nw), indexing="ij")
    return v.ravel(), omega.ravel()


def tree_pose_checks(res, branch, steps):
    """the poses a tree's call looked at: per node under a parent that took every step, its own free steps and the colliding pose"""
    n_nodes, _, _, offsets = K.arc_tree_nodes(branch, steps)
    free = res[:, 0].astype(np.int64)
    total, before, parent_free = 0, 0, np.zeros(1, dtype=np.int64)
    for e, (b, n) in enumerate(zip(branch, steps)):
        end = offsets[e + 1] if e + 1 < len(branch) else n_nodes
        own = free[offsets[e]:end] - np.repeat(parent_free, b)
        rolled = np.repeat(parent_free == before, b)  # the parent is alive
        total += int(np.minimum(own[rolled] + 1, n).sum())
        parent_free, before = free[offsets[e]:end], before + n
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    bind, where = placement()
    if bind:
        bind()
    weight = K.plan_weights()
    c = cases(a.frames, only=[("cfg1", 0.05)])[0]
    grid, cfg = c["grid"], c["cfg"]
    costmap, _, goal, _ = plan(c, weight)
    potential = grid.potential(c["table"], weight, [goal], **KW)  # leaves the plan
    q = K.plan_q(costmap, weight)
    pose = c["pose"]
    start = K.arc_start(pose[4], pose[5], 2.0 * math.atan2(pose[2], pose[3]))
    footprint = K.footprint_box(*BOX)
    geometry = (cfg["cell"], cfg["origin_x"], cfg["origin_y"])
    open_grid, open_costmap = make_grid(cfg), np.zeros_like(costmap)
    open_potential = open_grid.potential_of_costmap(open_costmap, weight, [goal])
    open_q = K.plan_q(open_costmap, weight)
    runs = []
    for floor, (g, fq, fpot) in (("drive", (grid, q, potential)), ("open", (open_grid, open_q, open_potential))):
        for branch in TREES:
            steps = (LEVEL_STEPS,) * len(branch)
            n_nodes, n_leaves, total_steps, _ = K.arc_tree_nodes(branch, steps)
            commands = [level_commands(b) for b in branch]
            primitives = K.arc_steps(np.concatenate([v for v, _ in commands]), np.concatenate([w for _, w in commands]), DT)
            side = int(round(math.sqrt(n_leaves)))
            assert side * side == n_leaves
            v, omega = np.meshgrid(np.linspace(0.0, 1.5, side), np.linspace(-1.5, 1.5, side), indexing="ij")
            runs.append(dict(floor=floor, grid=g, q=fq, potential=fpot, branch=branch, steps=steps, primitives=primitives, flat_arcs=K.arc_steps(v.ravel(), omega.ravel(), DT),
                             n_nodes=n_nodes, n_leaves=n_leaves, total_steps=total_steps, dev=np.empty((n_nodes, 4), dtype=np.uint32),
                             host=np.empty((n_nodes, 4), dtype=np.uint32), flat=np.empty((n_leaves, 4), dtype=np.uint32), t={"device": [], "host": [], "flat": []}))
    for r in range(a.rounds + 3):  # (the first three rounds warm)
        for f in runs:
            host_too = f["floor"] == "drive" or r < 8
            t = [time.perf_counter()]
            f["grid"].score_arc_tree(start, f["branch"], f["steps"], f["primitives"], footprint, out=f["dev"])
            t.append(time.perf_counter())
            if host_too:
                K.score_arc_tree_from_plan(f["q"], f["potential"], *geometry, start, f["branch"], f["steps"], f["primitives"], footprint, out=f["host"])
            t.append(time.perf_counter())
            f["grid"].score_arcs(start, f["flat_arcs"], f["total_steps"], footprint, out=f["flat"])
            t.append(time.perf_counter())
            if r == 0:
                assert np.array_equal(f["dev"], f["host"])
                leaves = f["dev"][f["n_nodes"] - f["n_leaves"]:]
                best = K.arc_tree_best(f["dev"], f["branch"], f["steps"], w_potential=1, w_cost=1, w_blocked=1000)
                f["result"] = {"leaves_that_end_early_share": float((leaves[:, 0] < f["total_steps"]).mean()), "mean_free_steps_of_the_leaves": float(leaves[:, 0].mean()),
                               "tree_pose_checks": tree_pose_checks(f["dev"], f["branch"], f["steps"]),
                               "tree_pose_checks_at_most": int(sum(int(np.prod(f["branch"][:e + 1])) * n for e, n in enumerate(f["steps"]))),
                               "flat_pose_checks": int(np.minimum(f["flat"][:, 0].astype(np.int64) + 1, f["total_steps"]).sum()),
                               "flat_pose_checks_at_most": f["n_leaves"] * f["total_steps"],
                               "best_leaf": None if best is None else {"leaf": best[0], "path": list(best[1]), "result": leaves[best[0]].tolist()}}
            if r >= 3:
                for k, name in enumerate(("device", "host", "flat")):
                    if name != "host" or host_too:
                        f["t"][name].append((t[k + 1] - t[k]) * 1e3)
    rows = [{"floor": f["floor"], "branch": list(f["branch"]), "steps_per_level": LEVEL_STEPS, "launches": len(f["branch"]), "nodes": f["n_nodes"], "leaves": f["n_leaves"],
             "steps_along_a_path": f["total_steps"], "dt_s": DT, "footprint_samples": len(footprint), "host_rounds": len(f["t"]["host"]), **f["result"],
             "grid_score_arc_tree_ms": spread(f["t"]["device"]), "host_score_arc_tree_from_plan_ms": spread(f["t"]["host"]),
             "grid_score_arcs_of_as_many_leaves_and_steps_ms": spread(f["t"]["flat"]),
             "host_over_device": float(np.median(f["t"]["host"])) / float(np.median(f["t"]["device"])),
             "flat_fan_over_tree": float(np.median(f["t"]["flat"])) / float(np.median(f["t"]["device"]))} for f in runs]
    print(json.dumps({"caller_process": where, "rounds": a.rounds, "scene": c["name"], "frames": a.frames, "cell_m": c["cell"], "grid_cells": [cfg["width"], cfg["height"]],
                      "goal": list(goal), "start": [float(v) for v in start], "passable_cells": int((q > 0).sum()), "trees": rows}))


if __name__ == "__main__":
    main()
