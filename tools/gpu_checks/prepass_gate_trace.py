"""Reads a rocprofv3 kernel trace (csv) of bench.py and relates every fused launch to the pre-pass kernels of the following call.

   rocprofv3 --kernel-trace --output-format csv -d <dir> -o run -- python3 bench.py --steps 200 --no-cpu-baseline
   python3 tools/gpu_checks/prepass_gate_trace.py <dir>/run_kernel_trace.csv

For every chain2_kernel launch: its duration, and the start of the amp33_rows_kernel launch nearest to its own start (the first of
the nine pre-pass kernels of the next call), relative to that start.  Prints the distribution of those offsets, the durations of
the fused launches with and without a pre-pass start within NEAR_US of their own, and where the pre-pass ends inside the launch."""
import bisect
import csv
import glob
import os
import statistics
import sys

NEAR_US = 5.0
PRE = ("amp33_rows_kernel", "sel_hist_kernel", "sel_scan_kernel", "rowcorr_kernel", "chan_kernel")


def q(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p * len(v)))]


def dist(v):
    if not v:
        return "n=0"
    return "n=%d min %.1f p10 %.1f median %.1f p90 %.1f max %.1f" % (len(v), min(v), q(v, 0.1), statistics.median(v), q(v, 0.9), max(v))


def main():
    path = sys.argv[1]
    if not path.endswith(".csv"):
        path = sorted(glob.glob(path + "/**/*kernel_trace.csv", recursive=True))[0]
    rows = list(csv.DictReader(open(path)))
    k = [(r["Kernel_Name"], int(r["Start_Timestamp"]) / 1e3, int(r["End_Timestamp"]) / 1e3) for r in rows]   # us
    k.sort(key=lambda r: r[1])
    fused = [r for r in k if "chain2_kernel" in r[0]]
    amp = [r for r in k if "amp33_rows_kernel" in r[0]]
    gate = [r for r in k if "prepass_gate_kernel" in r[0]]
    last = [r for r in k if "chan_kernel" in r[0]]
    amp_s = [r[1] for r in amp]
    last_s = [r[1] for r in last]
    print("trace: %s" % os.path.basename(path))
    print("launches: %d fused, %d amp33_rows_kernel, %d prepass_gate_kernel" % (len(fused), len(amp), len(gate)))
    # steady state only: skip the launches of set-up and warm-up that have no pre-pass beside them
    offs, durs_near, durs_far, ends, durs = [], [], [], [], []
    for name, s, e in fused[5:]:
        i = bisect.bisect_left(amp_s, s - 50.0)
        if i >= len(amp_s) or amp_s[i] >= e:
            continue   # no pre-pass started beside this launch
        o = amp_s[i] - s
        offs.append(o)
        durs.append(e - s)
        (durs_near if abs(o) <= NEAR_US else durs_far).append(e - s)
        j = bisect.bisect_left(last_s, amp_s[i])
        if j < len(last):
            ends.append(last[j][2] - s)
    print("fused launches with a pre-pass beside them: %d" % len(offs))
    print("start of amp33_rows_kernel minus start of the fused launch it runs beside, us: " + dist(offs))
    edges = [-1e9, -5, 0, 5, 20, 50, 100, 1e9]
    for a, b in zip(edges, edges[1:]):
        n = sum(1 for o in offs if a <= o < b)
        print("   [%s, %s) us: %d" % ("-inf" if a < -1e8 else "%g" % a, "inf" if b > 1e8 else "%g" % b, n))
    print("fused duration, all such launches, us:          " + dist(durs))
    print("fused duration, pre-pass start within %g us:     %s" % (NEAR_US, dist(durs_near)))
    print("fused duration, pre-pass start further away:    " + dist(durs_far))
    print("end of the pre-pass (chan_kernel) after the fused start, us: " + dist(ends))
    if gate:
        print("prepass_gate_kernel duration, us: " + dist([e - s for _, s, e in gate]))
        fs = [r[1] for r in fused]
        go = []
        for _, s, e in gate:
            i = bisect.bisect_right(fs, e) - 1
            if i >= 0:
                go.append(e - fs[i])
        print("end of the gate after the start of the fused launch before it, us: " + dist(go))
    for n in PRE:
        d = [e - s for name, s, e in k if n in name]
        print("  %-20s duration us: %s" % (n, dist(d)))


if __name__ == "__main__":
    main()
