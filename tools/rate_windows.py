"""What the rate tools of the search options share (playout_cap_rate.py, forced_playouts_rate.py, gumbel_rate.py,
starts_rate.py): one engine at the BASELINE.json configs[1] shape, and the modes of an option timed in alternating
windows of the same process on the same box.  An option changes between runs only, so every window is a run of its
own: the slots of the previous window are given up (agz_slot_abandon), the mode is set on a run without a step yet,
the run is started, stepped through its prelude and a warm-up, and then K steps are timed, ending in a synchronise.

And what the tools that also measure against the parent commit share (puct_rate.py, explore_rate.py, surprise_rate.py):
two libraries cannot share a process, so every round runs one child process per tree, in an order that reverses every
round, and "off" on this tree is held against the spread of the parent's own windows."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--tower", type=int, default=10)
    ap.add_argument("--readouts", type=int, default=400)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--stagger", type=int, default=60, help="the bench stagger (games at mixed stages, as in bench.py)")
    ap.add_argument("--steps", type=int, default=100, help="timed steps per window")
    ap.add_argument("--pairs", type=int, default=3, help="rounds of the windows (the order reverses every round)")
    ap.add_argument("--warmup", type=int, default=10)
    return ap


def engine(args, **cfg):
    import alphago_jl_amd as ag
    eng = ag.Engine(board_size=args.board, tower_height=args.tower, games=args.games, num_readouts=args.readouts,
                    parallel_readouts=8, seed=1, record_capacity_games=2 * args.games + 64, **cfg)
    eng.init_synthetic(0)
    return eng


def set_stagger(eng, moves):
    eng._ck(eng.L.agz_debug_set_stagger(eng.h, moves))


def first_search_steps(args):
    """steps until every game of a fresh run is behind its first search"""
    return (args.readouts + 7) // 8 + 5


def windows_of(eng, args, modes, configure, collect, prelude, counts=None, profile=True):
    """configure(eng, mode) sets the stagger and the mode; counts(eng) reads the option's counter pair;
    collect(s0, s1, c0, c1, dt) gives the option's own columns of a window (stats and counts before and behind it)
    -> {mode: [columns of each of its windows]}"""
    out = {m: [] for m in modes}
    live = False
    for k in range(args.pairs):
        for mode in (modes if k % 2 == 0 else modes[::-1]):
            if live:
                for g in range(args.games):
                    eng.slot_abandon(g)
            eng.records_clear()
            eng.start(0)                      # a run without a step yet: stagger and setting may change here
            configure(eng, mode)
            eng.start(0)
            live = True
            eng.step(prelude + args.warmup)
            eng.sync()
            s0, c0 = eng.stats(), counts(eng) if counts else None
            if profile:
                eng.profile_search(True)
            t0 = time.perf_counter()
            eng.step(args.steps)
            eng.sync()
            dt = time.perf_counter() - t0
            w = dict(ms_per_step=round(1e3 * dt / args.steps, 4))
            if profile:                       # the five search kernels' time per step (bench.py's `search_kernels`)
                search_ms, search_steps = eng.profile_search_read()
                eng.profile_search(False)
                w["search_kernels_ms_per_step"] = round(float(sum(search_ms.values())) / max(search_steps, 1), 4)
                w["k_pre_us_per_step"] = round(1e3 * float(search_ms.get("k_pre", 0.0)) / max(search_steps, 1), 2)
                w["k_expand_us_per_step"] = round(1e3 * float(search_ms.get("k_expand", 0.0)) / max(search_steps, 1), 2)
            s1, c1 = eng.stats(), counts(eng) if counts else None
            moves = s1["positions"] - s0["positions"]
            w.update(moves=moves, moves_per_s=round(moves / dt, 1),
                     evals_per_move=round((s1["evals"] - s0["evals"]) / max(moves, 1), 2),
                     pool_short_searches=s1["pool_short_searches"] - s0["pool_short_searches"])
            w.update(collect(s0, s1, c0, c1, dt))
            out[mode].append(w)
    return out


def summary(windows, keys):
    """median and spread (max - min) over a mode's windows of every column in `keys`"""
    res = {}
    for mode, ws in windows.items():
        res[mode] = {}
        for key in keys:
            v = [w[key] for w in ws]
            res[mode][key] = dict(median=round(statistics.median(v), 4), spread=round(max(v) - min(v), 4))
    return res


def on_minus_off(res, key):
    return round(res["on"][key]["median"] - res["off"][key]["median"], 4)


def measured(res):
    """on against off, beside the off windows' own spread"""
    return dict(ms_per_step_on_minus_off=on_minus_off(res, "ms_per_step"),
                search_kernels_on_minus_off=on_minus_off(res, "search_kernels_ms_per_step"),
                off_spread_ms_per_step=res["off"]["ms_per_step"]["spread"],
                off_spread_search_kernels=res["off"]["search_kernels_ms_per_step"]["spread"])


# ---------------------------------------------------------------- this tree against a built checkout of the parent

def parent_args(ap, child_timeout=900, data=True):
    """the arguments of a tool with a parent part (data: and of a data part at a small shape)"""
    ap.add_argument("--child", action="store_true", help="(internal) time one tree's windows and print them")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit; none: no parent part")
    ap.add_argument("--child-timeout", type=int, default=child_timeout)
    if data:
        ap.add_argument("--data-tower", type=int, default=2)
        ap.add_argument("--data-readouts", type=int, default=100)
        ap.add_argument("--data-games", type=int, default=256)
        ap.add_argument("--no-data", action="store_true")


def child_argv(args, names):
    """the arguments `names` of this process, as a child's command line"""
    return [x for k in names for x in ("--" + k.replace("_", "-"), str(getattr(args, k)))]


def run_child(script, tag, tree, argv, timeout):
    """`script --child --tree tree argv` in a process of its own -> what it printed as JSON behind `tag`; argv begins
    with the modes of the child (--modes M), which name it in the progress line and in a failure"""
    cmd = [sys.executable, os.path.abspath(script), "--child", "--tree", tree] + list(argv)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"child on {tree} ({argv[1]}) failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [x for x in r.stdout.splitlines() if x.startswith(tag + " ")][-1]
    print(f"windows of {tree} ({argv[1]}) done", file=sys.stderr, flush=True)
    return json.loads(line[len(tag) + 1:])


def parent_rounds(pairs, parent_tree, run_parent, run_this):
    """`pairs` rounds of run_parent(parent_tree) -> the parent's off windows and run_this(k) -> {off, on} windows of this
    tree, the parent first in the even rounds and last in the odd ones; without a parent tree only this tree runs
    -> {parent_off, off, on}"""
    windows = dict(parent_off=[], off=[], on=[])
    for k in range(pairs):
        for which in (("parent", "this") if k % 2 == 0 else ("this", "parent")):
            if which == "this":
                w = run_this(k)
                windows["off"] += w["off"]
                windows["on"] += w["on"]
            elif parent_tree:
                windows["parent_off"] += run_parent(parent_tree)
    return windows


def window_rounds(script, tag, args):
    """parent_rounds of a tool whose child times windows_of(): off on the parent; off and on, then on and off, on this"""
    def run(tree, modes):
        argv = ["--modes", modes, "--pairs", "1"] + child_argv(args, ("board", "tower", "readouts", "games", "stagger", "steps", "warmup"))
        return run_child(script, tag, tree, argv, args.child_timeout)
    this = os.path.dirname(os.path.dirname(os.path.abspath(script)))
    return parent_rounds(args.pairs, args.parent_tree, lambda tree: run(tree, "off")["off"],
                         lambda k: run(this, "off,on" if k % 2 == 0 else "on,off"))


def off_against_parent(res, keys):
    """keys = {name: (column, digits)}: off minus parent of the medians of every column, rounded to its digits, the
    parent's own spread beside it, and whether every difference lies inside that spread"""
    d = {k: round(res["off"][col]["median"] - res["parent_off"][col]["median"], nd) for k, (col, nd) in keys.items()}
    out = {"off_minus_parent_" + k: v for k, v in d.items()}
    out.update({"parent_spread_" + k: res["parent_off"][col]["spread"] for k, (col, _) in keys.items()})
    out["off_within_parent_spread"] = all(abs(d[k]) <= res["parent_off"][col]["spread"] for k, (col, _) in keys.items())
    return out
