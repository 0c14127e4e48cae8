#!/usr/bin/env python3
"""Idle time between the kernels of one sort, from a rocprofv3 kernel trace (the *_kernel_trace.csv of tools/profile.sh's
`trace` pass): per sort, first kernel start -> last kernel end against the sum of the kernel durations.

    tools/trace_gaps.py <trace dir> [passes]      a sort = joint_histograms ... the passes-th rank_scatter after it
    tools/trace_gaps.py <trace dir> --hybrid      a sort = the opening clear ... finish_plan, of sorts that try the hybrid form

--hybrid: only the sorts in which the hybrid form ran (a local_sort_kernel of 60 us or more) and of the size that occurs most
(bench.py's measured steps; warm-up sorts of the same size are among them).  Printed: the launches per sort, the medians of span,
of the working kernels (the upfront read, the global passes and the local stage that ran: everything of 60 us or more), of all the
other launches together and of the idle time; then the median sort launch by launch."""
import csv, glob, statistics, sys

WORKING_US = 60.0   # a launch that returns at once takes 4 to 16 us; the shortest working kernel of a 2^24-key sort 100


def read_rows(path):
    rows = []
    for f in glob.glob(path + "/**/*kernel_trace.csv", recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def short(name):
    name = name.replace("lsd::", "").replace("void ", "")
    return name[:72]


def print_sort(c):
    prev = None
    for s, e, name in c:
        gap = "" if prev is None else f"  (+{(s - prev)/1e3:.1f} us after the previous kernel)"
        print(f"  {short(name):72s} {(e - s)/1e3:8.1f} us{gap}")
        prev = e


def by_passes(rows, passes):
    # a sort = joint_histograms ... 4th rank_scatter after it
    sorts, cur = [], None
    for s, e, name in rows:
        if "joint_histograms" in name:
            cur = [(s, e, name)]
        elif cur is not None:
            cur.append((s, e, name))
            if sum("rank_scatter" in n for _, _, n in cur) == passes:
                sorts.append(cur)
                cur = None
    if not sorts:
        sys.exit("no sorts found")
    span = [c[-1][1] - c[0][0] for c in sorts]
    busy = [sum(e - s for s, e, _ in c) for c in sorts]
    print(f"{len(sorts)} sorts: span median {statistics.median(span)/1e3:.1f} us, kernels {statistics.median(busy)/1e3:.1f} us, "
          f"idle between kernels {statistics.median([a - b for a, b in zip(span, busy)])/1e3:.1f} us")
    print_sort(sorts[len(sorts) // 2])


def by_hybrid(rows):
    # a sort = clear_kernel ... finish_plan_kernel, with a hybrid_sample_kernel in between (the form was tried)
    sorts, cur = [], None
    for row in rows:
        name = row[2]
        if "clear_kernel" in name and "_clear_kernel" not in name:
            cur = [row]
        elif cur is not None:
            cur.append(row)
            if "finish_plan_kernel" in name:
                if any("hybrid_sample_kernel" in n for _, _, n in cur):
                    sorts.append(cur)
                cur = None
    ran = [c for c in sorts if any("local_sort_kernel" in n and (e - s) / 1e3 >= WORKING_US for s, e, n in c)]
    if not ran:
        sys.exit("no sort in which the hybrid form ran")
    # the size that occurs most: by the upfront read's duration, to 5 %, and the launch count
    def shape(c):
        up = max((e - s for s, e, n in c if "hybrid_histograms_kernel" in n), default=0)
        return (len(c), round(20 * up / max(up for cc in ran for s, e, n in cc if "hybrid_histograms_kernel" in n)))
    shapes = [shape(c) for c in ran]
    most = max(set(shapes), key=shapes.count)
    picked = [c for c, sh in zip(ran, shapes) if sh == most]
    us = lambda x: x / 1e3
    span = [us(c[-1][1] - c[0][0]) for c in picked]
    work = [sum(us(e - s) for s, e, _ in c if us(e - s) >= WORKING_US) for c in picked]
    rest = [sum(us(e - s) for s, e, _ in c if us(e - s) < WORKING_US) for c in picked]
    idle = [a - b - r for a, b, r in zip(span, work, rest)]
    nwork = statistics.median([sum(us(e - s) >= WORKING_US for s, e, _ in c) for c in picked])
    med = statistics.median
    print(f"{len(sorts)} sorts tried the hybrid form, it ran in {len(ran)}; {len(picked)} of the most frequent shape: "
          f"{most[0]} launches per sort, {nwork:g} of them working kernels (>= {WORKING_US:g} us)")
    print(f"medians per sort: span {med(span):.1f} us = working kernels {med(work):.1f} + other launches {med(rest):.1f} + idle {med(idle):.1f};"
          f"  span - working kernels {med([a - b for a, b in zip(span, work)]):.1f} us")
    names = [n for _, _, n in picked[0]]
    if all([n for _, _, n in c] == names for c in picked):
        print("median duration of every launch, in order:")
        for i, n in enumerate(names):
            d = med([us(c[i][1] - c[i][0]) for c in picked])
            g = med([us(c[i][0] - c[i - 1][1]) for c in picked]) if i else 0.0
            mark = "*" if d >= WORKING_US else " "
            print(f" {mark}{short(n):72s} {d:8.1f} us   (+{g:.1f} us after the previous kernel)")
    print("the median sort (by span):")
    print_sort(sorted(picked, key=lambda c: c[-1][1] - c[0][0])[len(picked) // 2])


if __name__ == "__main__":
    rows = read_rows(sys.argv[1])
    if len(sys.argv) > 2 and sys.argv[2] == "--hybrid":
        by_hybrid(rows)
    else:
        by_passes(rows, int(sys.argv[2]) if len(sys.argv) > 2 else 4)
