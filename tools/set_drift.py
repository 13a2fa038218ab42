"""Do the dispatch sets of a step group run independently?  From a `rocprofv3 --kernel-trace --output-format csv` run of bench.py.

    python tools/set_drift.py <kernel_trace.csv> [--last N]

For every stream that ran `k_avoiding_step_split`: queue, workgroups and the duration distribution of its last N dispatches (default 300: the timed region of
the default bench command).  For the first two such streams with at least N dispatches: start of dispatch i on the second minus start of dispatch i on the
first, i counted from the end - first value, last value, minimum, maximum, and the standard deviation of its step-to-step change.  Independent sets WANDER
(the offset moves by the difference of the two dispatch durations every step); a constant offset means that the sets are coupled, e.g. through a shared
hardware queue.  All figures in microseconds.
"""
import argparse
import csv
import statistics
from collections import defaultdict


def dist(xs):
    xs = sorted(xs)
    q = lambda p: xs[min(len(xs) - 1, int(p * len(xs)))]
    return "mean %.1f median %.1f p10 %.1f p90 %.1f" % (statistics.fmean(xs), q(0.5), q(0.1), q(0.9))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("trace")
    ap.add_argument("--last", type=int, default=300)
    args = ap.parse_args()
    by_stream = defaultdict(list)
    with open(args.trace, newline="") as f:
        for r in csv.DictReader(f):
            if "k_avoiding_step_split" in r["Kernel_Name"]:
                by_stream[r["Stream_Id"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"],
                                                  int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))))
    full = []
    for sid, rs in sorted(by_stream.items()):
        rs.sort()
        last = rs[-args.last:]
        print("stream %s: %d dispatches in all; last %d: queues %s, workgroups %s, duration %s"
              % (sid, len(rs), len(last), sorted(set(r[2] for r in last)), sorted(set(r[3] for r in last)), dist([(r[1] - r[0]) / 1e3 for r in last])))
        if len(rs) >= args.last:
            full.append((sid, last))
    if len(full) < 2:
        print("fewer than two streams with %d step dispatches: nothing to compare" % args.last)
        return
    (sa, a), (sb, b) = full[0], full[1]
    off = [(y[0] - x[0]) / 1e3 for x, y in zip(a, b)]
    d = [q - p for p, q in zip(off[:-1], off[1:])]
    print("start of dispatch i on stream %s minus on stream %s: first %.1f last %.1f min %.1f max %.1f; step-to-step change: stdev %.1f, mean |change| %.1f"
          % (sb, sa, off[0], off[-1], min(off), max(off), statistics.pstdev(d), statistics.fmean(abs(x) for x in d)))
    k = max(1, len(off) // 10)
    print("every %dth offset: %s" % (k, " ".join("%.0f" % x for x in off[::k])))


if __name__ == "__main__":
    main()
