"""Per-queue idle time around the Avoiding step kernel, from a `rocprofv3 --kernel-trace --output-format csv` run of bench.py.

    python tools/queue_idle.py <kernel_trace.csv> [--last N] [--skip K] [--reset-us T]

For every hardware queue that ran `k_avoiding_step_split`, the last N step dispatches of each of its streams (the timed region of the default bench command
is the last 300 per stream; several streams may share one hardware queue) are walked in start order.  --skip K leaves out the last K per stream first:
`--skip 300 --last 250` is the untimed pre-roll of the same run, where no event records surround the step launch.
Between two step dispatches the queue ran either nothing (one launch per step) or the tail kernel:
  gap_step_tail   tail start - step end          (queue idle between the step kernel and the tail)
  gap_tail_step   next step start - tail end     (queue idle between the tail and the next step kernel)
  gap_step_step   next step start - step end     (one launch per step: the whole idle time of a period)
  tail            tail end - tail start, split at --reset-us: a tail that resets no lane runs no forward-dynamics pass and stays below it.  The trace
                  does not say which lanes finished; the split is by duration.
  period          step start to next step start
All figures in microseconds: mean / median / p10 / p90 over the dispatches of all queues, and the per-queue means.
"""
from __future__ import annotations

import argparse
import csv
import json
import statistics
from collections import defaultdict


def _col(header, *names):
    low = [h.strip().lower() for h in header]
    for n in names:
        if n in low:
            return low.index(n)
    raise SystemExit("column %s not in %s" % (names, header))


def load(path):
    with open(path, newline="") as f:
        rd = csv.reader(f)
        header = next(rd)
        iq, ik, istream = _col(header, "queue_id"), _col(header, "kernel_name"), _col(header, "stream_id")
        i0, i1 = _col(header, "start_timestamp"), _col(header, "end_timestamp")
        by_queue = defaultdict(list)
        for row in rd:
            if len(row) <= max(iq, ik, i0, i1):
                continue
            by_queue[row[iq]].append((int(row[i0]), int(row[i1]), row[ik], row[istream]))
    return by_queue


def summarize(xs):
    if not xs:
        return None
    xs = sorted(xs)
    q = lambda p: xs[min(len(xs) - 1, int(p * len(xs)))]
    return {"n": len(xs), "mean": round(statistics.fmean(xs), 2), "median": round(q(0.5), 2), "p10": round(q(0.1), 2), "p90": round(q(0.9), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--last", type=int, default=300, help="step dispatches per queue to look at, counted from the end of the trace")
    ap.add_argument("--skip", type=int, default=0, help="leave out this many step dispatches per stream at the end of the trace first")
    ap.add_argument("--reset-us", type=float, default=5.0, help="a tail at least this long is counted as one that reset a lane")
    ap.add_argument("--json", default=None, help="also write the table here")
    args = ap.parse_args()
    rows = defaultdict(list)
    per_queue = {}
    for qid, ds in sorted(load(args.trace).items()):
        ds.sort()
        steps = [i for i, d in enumerate(ds) if "k_avoiding_step_split" in d[2]]
        if len(steps) < 2:
            continue
        t_lo, t_hi = 0, float("inf")      # the window in time: where every stream of the queue is inside its [-(skip + last + 1), -skip) step dispatches
        for sid in sorted(set(ds[i][3] for i in steps)):
            own = [ds[i][0] for i in steps if ds[i][3] == sid]
            if args.skip and len(own) >= args.skip:
                t_hi = min(t_hi, own[-args.skip])
            t_lo = max(t_lo, own[max(0, len(own) - args.skip - args.last - 1)])
        steps = [i for i in steps if t_lo <= ds[i][0] < t_hi]
        if len(steps) < 2:
            continue
        mine = defaultdict(list)
        for a, b in zip(steps[:-1], steps[1:]):
            s0, s1 = ds[a], ds[b]
            mine["step"].append((s0[1] - s0[0]) / 1e3)
            mine["period"].append((s1[0] - s0[0]) / 1e3)
            mine["dispatches_per_step"].append(b - a)
            between = ds[a + 1:b]
            tails = [d for d in between if "k_avoiding_tail" in d[2]]
            if len(between) == 1 and tails:
                t = tails[0]
                mine["gap_step_tail"].append((t[0] - s0[1]) / 1e3)
                mine["gap_tail_step"].append((s1[0] - t[1]) / 1e3)
                dur = (t[1] - t[0]) / 1e3
                mine["tail_reset" if dur >= args.reset_us else "tail_no_reset"].append(dur)
                mine["idle"].append((s1[0] - s0[1]) / 1e3 - dur)
            elif not between:
                mine["gap_step_step"].append((s1[0] - s0[1]) / 1e3)
                mine["idle"].append((s1[0] - s0[1]) / 1e3)
            else:
                mine["other_between"].append(len(between))
        per_queue[qid] = {k: round(statistics.fmean(v), 2) for k, v in mine.items()}
        for k, v in mine.items():
            rows[k] += v
    out = {"queues": len(per_queue), "all": {k: summarize(v) for k, v in rows.items()}, "per_queue_mean": per_queue}
    print("%-20s %6s %9s %9s %9s %9s" % ("us", "n", "mean", "median", "p10", "p90"))
    for k, s in out["all"].items():
        print("%-20s %6d %9.2f %9.2f %9.2f %9.2f" % (k, s["n"], s["mean"], s["median"], s["p10"], s["p90"]))
    for qid, m in per_queue.items():
        print("queue %s: %s" % (qid, json.dumps(m)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
