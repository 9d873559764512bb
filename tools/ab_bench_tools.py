"""Bench tools of this repository on a tree of the parent commit against this tree, alternating processes on one box.
    python tools/ab_bench_tools.py --parent-root DIR [--tools bench_open_system.py,bench_determined.py] [--pairs 5] --out FILE.json
DIR is a checkout of the parent commit with its library built (its tools, tests and k16.py are the ones its side runs).  Per
tool and pair one fresh process per side, the parent first; each writes its own JSON (--out of the tool), from which every
`p50_of_runs_ms` table -- at the top level or one level down, where a tool benches several circuits -- and the p50 of a
`depth_leg` are read.  Per leg: this tree's p50 over the pairs against the parent's p50 and the parent's lowest and highest
run, and the legs whose tree p50 lies outside that spread.  Output: --out, and the same as text on stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def legs_of(j):
    """{leg: ms} of one process's JSON"""
    r = {}
    for leg, v in j.get("p50_of_runs_ms", {}).items():
        r[leg] = v
    for name, sub in j.items():
        if isinstance(sub, dict) and isinstance(sub.get("p50_of_runs_ms"), dict):
            for leg, v in sub["p50_of_runs_ms"].items():
                r["%s.%s" % (name, leg)] = v
    if isinstance(j.get("depth_leg"), dict) and "p50_ms" in j["depth_leg"]:
        r["depth_leg"] = j["depth_leg"]["p50_ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--tools", default="bench_open_system.py,bench_determined.py")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per process")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    out, outside = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for tool in args.tools.split(","):
            runs = {"parent": [], "tree": []}
            for pair in range(args.pairs):
                for side, root in (("parent", args.parent_root), ("tree", ROOT)):
                    path = os.path.join(tmp, "%s_%s_%d.json" % (tool, side, pair))
                    subprocess.run([sys.executable, os.path.join(root, "tools", tool), "--out", path], check=True, timeout=args.timeout,
                                   stdout=subprocess.DEVNULL)
                    runs[side].append(legs_of(json.load(open(path))))
                print("%s pair %d done" % (tool, pair), flush=True)
            legs, parts = {}, []
            for leg in runs["parent"][0]:
                if leg not in runs["tree"][0]:
                    continue
                p, t = [r[leg] for r in runs["parent"]], [r[leg] for r in runs["tree"]]
                tp, pp, lo, hi = statistics.median(t), statistics.median(p), min(p), max(p)
                legs[leg] = {"tree_p50_ms": tp, "parent_p50_ms": pp, "parent_lowest_ms": lo, "parent_highest_ms": hi, "tree_runs_ms": t, "parent_runs_ms": p}
                parts.append("`%s` %.4f against %.4f (%.4f-%.4f)" % (leg, tp, pp, lo, hi))
                if tp < lo or tp > hi:
                    outside.append("`%s` of `%s`, %.4f against %.4f-%.4f (%+.1f %% of the parent's p50)" % (leg, tool, tp, lo, hi, 100 * (tp - pp) / pp))
            out[tool] = {"pairs": args.pairs, "legs": legs}
            print("`tools/%s` (%d pairs): %s" % (tool, args.pairs, ", ".join(parts)))
    print("outside the parent's spread: " + ("; ".join(outside) if outside else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
