"""diagnostics: the kernel boundary as the patch launches pay it -- end-to-start gap between consecutive dispatches of
the patch kernel on the same queue, from a rocprofv3 --kernel-trace CSV (tools/prof_edges.sh writes one).
usage: python tools/launch_gaps.py <..._kernel_trace.csv> [kernel name substring, default k_patch_]"""
import csv
import statistics
import sys


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "k_patch_"
    rows = list(csv.DictReader(open(path)))
    by_queue = {}
    for r in rows:
        by_queue.setdefault(r["Queue_Id"], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    gaps, durs = [], []
    for q in by_queue.values():
        q.sort()
        for (s0, e0, n0), (s1, e1, n1) in zip(q, q[1:]):
            if want in n0 and want in n1:
                gaps.append((s1 - e0) / 1e3)
        durs += [(e - s) / 1e3 for s, e, n in q if want in n]
    if not gaps:
        print("no consecutive", want, "dispatches in", path)
        return
    gaps.sort()
    pct = lambda v, f: v[min(len(v) - 1, int(f * len(v)))]
    print("%s: %d dispatches, duration us mean %.2f median %.2f" % (want, len(durs), statistics.mean(durs), statistics.median(durs)))
    print("end-to-start gap on the same queue, us: n %d mean %.2f median %.2f p10 %.2f p90 %.2f max %.2f" %
          (len(gaps), statistics.mean(gaps), statistics.median(gaps), pct(gaps, 0.1), pct(gaps, 0.9), gaps[-1]))


if __name__ == "__main__":
    main()
