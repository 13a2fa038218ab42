"""Which hardware queue ran the Avoiding step dispatches of which stream, and how large they were, from a `rocprofv3 --kernel-trace --output-format csv` run
of bench.py.  What `tools/queue_idle.py` does not print: the stream -> queue mapping and the grid of the dispatches.

    python tools/step_dispatches.py <kernel_trace.csv> [--last N]

--last: the dispatches per stream that are looked at, counted from the end (default 300: the timed region of the default bench command).
"""
import argparse
import csv
from collections import Counter, defaultdict


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("trace")
    ap.add_argument("--last", type=int, default=300)
    args = ap.parse_args()
    by_stream = defaultdict(list)
    with open(args.trace, newline="") as f:
        for r in csv.DictReader(f):
            if "k_avoiding_step_split" in r["Kernel_Name"]:
                by_stream[r["Stream_Id"]].append(r)
    for sid, rs in sorted(by_stream.items()):
        rs.sort(key=lambda r: int(r["Start_Timestamp"]))
        last = rs[-args.last:]
        q = Counter(r["Queue_Id"] for r in last)
        wg = Counter((int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"])), int(r["Workgroup_Size_X"])) for r in last)
        names = Counter(r["Kernel_Name"][:60] for r in last)
        dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in last]
        print("stream %s: %d step dispatches in all; last %d: queues %s, (workgroups, threads) %s, mean %.1f us, kernels %s"
              % (sid, len(rs), len(last), dict(q), dict(wg), sum(dur) / len(dur), dict(names)))


if __name__ == "__main__":
    main()
