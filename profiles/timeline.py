"""One timed step's kernel timeline from a rocprofv3 --kernel-trace run of bench.py --profile-phase.

  python3 profiles/timeline.py <dir with *kernel_trace.csv> [anchor kernel substring]

Steps are cut at each dispatch of the anchor kernel: the first kernel of a step on the caller's
stream. The default, k_input_stats, fits steps without a lookahead (the cold phase's first steps,
plans of towers without BatchNorm); a steady-state plan step prepared its input statistics one step
ahead and starts with the conv-1 forward -- pass "k_conv_rows<0, 0," (fp16 tracks) for those, as
profiles/gpu_only_timeline.sh does. Prints the median step period, then the kernels of the step
whose period is the median (start offset, duration, queue), each queue's busy time (union of its
kernels' intervals over the period), the median gap before each kernel of the anchor queue, the
wrap-around gap (last anchor-queue kernel of step t -> the anchor of step t+1, which the per-step
gaps cannot show), conv 2's start offset, and for each side-queue consumer of a cross-queue edge its
start lag behind the latest end of its producers (EDGES).
"""
import csv
import glob
import os
import statistics
import sys

MARK = "spin_kernel"
DGRAD = "k_conv_rows<1,"  # the input gradients on the anchor queue, in issue order: dgrad 5, 4, 3, 2
# The plan step's cross-queue edges: (label, consumer name prefixes -- its first dispatch off the
# anchor queue --, producers: ("dgrad", index into the step's dgrads) or ("name", substring: every
# dispatch of the step off the anchor queue))
EDGES = [
    ("dgrad 4 -> layer 3-5 weight gradients", ("k_conv_wgrad16_multi", "k_conv_wgrad_multi"), [("dgrad", 1)]),
    ("dgrad 4 -> user-tower backward", ("k_tgemm2",), [("dgrad", 1)]),
    ("dgrad 3 -> layer-2 weight gradient", ("k_conv_wgrad16t", "k_conv_wgrad16<", "k_conv_wgrad<"), [("dgrad", 2)]),
    ("weight-gradient reduces + user-table Adam -> late Adam", ("k_adam_dense_pack",),
     [("name", "k_wgrad_reduce_multi"), ("name", "k_emb_grad_adam"), ("name", "k_adam_touched")]),
]


def short_name(n):
    return n.split("(")[0].replace("void ", "").replace("dcue::", "")


def edge_lags(ks, starts, q_anchor):
    """Per edge, over every whole step: consumer start - latest producer end (us)."""
    lags = {e[0]: [] for e in EDGES}
    for j in range(len(starts) - 1):
        t0, t1 = starts[j], starts[j + 1]
        step = [k for k in ks if t0 <= k[0] < t1]
        dgrads = [k for k in step if k[3] == q_anchor and DGRAD in k[2]]
        for label, consumers, producers in EDGES:
            prod = []
            for kind, what in producers:
                if kind == "dgrad":
                    prod += dgrads[what:what + 1] if len(dgrads) == 4 else []
                else:
                    prod += [k for k in step if k[3] != q_anchor and what in k[2]]
            if not prod:
                continue
            first, ends = min(k[0] for k in prod), [k[1] for k in prod]
            # (the late Adam may start after the next step has: look one period further)
            c = next((k for k in ks if k[3] != q_anchor and first <= k[0] < t1 + (t1 - t0)
                      and short_name(k[2]).startswith(consumers)), None)
            if c is not None:
                lags[label].append((c[0] - max(ends)) / 1e3)
    return lags


def main():
    d = sys.argv[1]
    anchor = sys.argv[2] if len(sys.argv) > 2 else "k_input_stats"
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    ks = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "?"))
                 for r in rows), key=lambda x: x[0])
    marks = [k for k in ks if MARK in k[2]]
    if len(marks) >= 2:
        lo, hi = marks[0][1], marks[-1][0]
        ks = [k for k in ks if k[0] >= lo and k[1] <= hi and MARK not in k[2]]
    starts = [k[0] for k in ks if anchor in k[2]]
    periods = [(starts[i + 1] - starts[i], i) for i in range(len(starts) - 1)]
    if not periods:
        print("no anchor dispatches")
        return
    med = statistics.median(p for p, _ in periods)
    print("steps %d  period median %.1f us  min %.1f  max %.1f" % (
        len(periods), med / 1e3, min(periods)[0] / 1e3, max(periods)[0] / 1e3))
    per, i = min(periods, key=lambda x: abs(x[0] - med))
    t0, t1 = starts[i], starts[i + 1]
    step = [k for k in ks if t0 <= k[0] < t1]
    q_anchor = next(k[3] for k in step if anchor in k[2])
    busy = {}
    for s, e, n, q in step:
        busy.setdefault(q, []).append((s, min(e, t1)))
    print("%8s %8s %6s  %s" % ("start", "dur", "queue", "kernel"))
    for s, e, n, q in step:
        short = n.split("(")[0].replace("void ", "").replace("dcue::", "")
        print("%8.1f %8.1f %6s%s %s" % ((s - t0) / 1e3, (e - s) / 1e3, q, "*" if q == q_anchor else " ", short[:90]))
    for q, iv in busy.items():
        iv.sort()
        tot, cs, ce = 0, None, None
        for s, e in iv:
            if cs is None or s > ce:
                if cs is not None:
                    tot += ce - cs
                cs, ce = s, e
            else:
                ce = max(ce, e)
        tot += ce - cs
        print("queue %s busy %.1f us of %.1f (%.0f%%)" % (q, tot / 1e3, per / 1e3, 100.0 * tot / per))
    # the anchor queue over every step: median gap before each of its kernels (by position in the
    # step) -- what cross-stream waits, event records and dispatch cost the critical chain
    gaps = {}
    for j in range(len(starts) - 1):
        a, b = starts[j], starts[j + 1]
        chain = [k for k in ks if a <= k[0] < b and k[3] == q_anchor]
        for n, (k0, k1) in enumerate(zip(chain, chain[1:])):
            name = k1[2].split("(")[0].replace("void ", "").replace("dcue::", "")[:60]
            gaps.setdefault((n, name), []).append((k1[0] - k0[1]) / 1e3)
    print("anchor-queue gaps (median over %d steps, us):" % (len(starts) - 1))
    tot = 0.0
    for (n, name), v in sorted(gaps.items()):
        g = statistics.median(v)
        tot += g
        print("  %6.1f  before %s" % (g, name))
    print("  %6.1f  total" % tot)
    # what the per-step gaps leave out: the end of a step's last kernel on the anchor queue to the
    # next step's anchor
    wrap, conv2 = [], []
    for j in range(len(starts) - 1):
        a, b = starts[j], starts[j + 1]
        chain = [k for k in ks if a <= k[0] < b and k[3] == q_anchor]
        wrap.append((b - max(k[1] for k in chain)) / 1e3)
        fwd = [k for k in chain if "k_conv_rows<0," in k[2]]
        if len(fwd) > 1:
            conv2.append((fwd[1][0] - a) / 1e3)
    print("wrap-around gap (last anchor-queue kernel -> next anchor): median %.1f us  min %.1f  max %.1f" % (
        statistics.median(wrap), min(wrap), max(wrap)))
    if conv2:
        print("conv 2 start offset: median %.1f us" % statistics.median(conv2))
    print("side-queue consumer lag behind the latest producer end (median over the steps, us):")
    for label, v in edge_lags(ks, starts, q_anchor).items():
        if v:
            print("  %6.1f  %s  (min %.1f, max %.1f, %d steps)" % (statistics.median(v), label, min(v), max(v), len(v)))
        else:
            print("       -  %s  (not found)" % label)


if __name__ == "__main__":
    main()
