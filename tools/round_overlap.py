"""Overlap of consecutive rounds of a pipelined step group (group option "pipeline_depth"), from a `rocprofv3 --kernel-trace
--output-format csv` run of bench.py.

    python tools/round_overlap.py <kernel_trace.csv> [--last N]

The step dispatches of ALL streams in start order are the rounds (one dispatch per round under one dispatch set).  Over the last N of them (default 300:
the timed region of the default bench command), in microseconds:
  queues      the hardware queue of every round: the rotation (e.g. 2 3 4 2 3 4) and how many rounds broke it
  overlap     end of round r - start of round r + 1; positive: round r + 1 was on the chip before round r had ended
  period      start of round r + 1 - start of round r, and (end of the last round - end of the first) / (N - 1): the step period of the region
  duration    start to end of a round: it includes the time the round's workgroups waited for their predecessors
  lead        start of round r + 1 to end of round r where positive: the longest wait a workgroup of round r + 1 can have had for round r (the figure
              "pipeline_timeout_ms" is a large multiple of)
"""
import argparse
import csv
import statistics
from collections import Counter


def _summ(xs):
    xs = sorted(xs)
    q = lambda p: xs[min(len(xs) - 1, int(p * len(xs)))]
    return "mean %.1f median %.1f p10 %.1f p90 %.1f min %.1f max %.1f" % (statistics.fmean(xs), q(0.5), q(0.1), q(0.9), xs[0], xs[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("trace")
    ap.add_argument("--last", type=int, default=300)
    args = ap.parse_args()
    rounds = []
    with open(args.trace, newline="") as f:
        for r in csv.DictReader(f):
            if "k_avoiding_step_split" in r["Kernel_Name"]:
                rounds.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], r["Stream_Id"], r["Kernel_Name"][:64],
                               int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))))
    rounds.sort()
    last = rounds[-args.last:]
    if len(last) < 3:
        raise SystemExit("fewer than three step dispatches in the trace")
    print("%d step dispatches in all; last %d: kernels %s, workgroups %s" % (len(rounds), len(last), dict(Counter(r[4] for r in last)), dict(Counter(r[5] for r in last))))
    qs = [r[2] for r in last]
    distinct = sorted(set(qs))
    cycle = qs[:len(distinct)]
    broke = sum(1 for i, q in enumerate(qs) if q != cycle[i % len(cycle)])
    print("queues      %s (streams %s); first rounds %s; rounds off the rotation of the first %d: %d" % (dict(Counter(qs)), dict(Counter(r[3] for r in last)), " ".join(qs[:9]), len(cycle), broke))
    us = lambda a: a / 1e3
    overlap = [us(a[1] - b[0]) for a, b in zip(last[:-1], last[1:])]
    print("overlap     %s; rounds that started before their predecessor ended: %d of %d" % (_summ(overlap), sum(1 for x in overlap if x > 0), len(overlap)))
    print("period      %s; by the ends of the region: %.2f" % (_summ([us(b[0] - a[0]) for a, b in zip(last[:-1], last[1:])]), us(last[-1][1] - last[0][1]) / (len(last) - 1)))
    print("duration    %s" % _summ([us(r[1] - r[0]) for r in last]))
    lead = [x for x in overlap if x > 0]
    print("lead        %s" % (_summ(lead) if lead else "no round overlapped its predecessor"))


if __name__ == "__main__":
    main()
