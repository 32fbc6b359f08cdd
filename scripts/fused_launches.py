"""The fused launches of the last tgsim_step_n call in a rocprofv3 kernel trace (--kernel-trace, csv)
of a plain storm bench: each k_sim_fused launch's duration, the gaps between consecutive launches,
and the drain (from the end of the last k_sim_fused to the end of the last kernel of the trace's
timed region, i.e. the last group's delivery).  usage: fused_launches.py kernel_trace.csv N_LAUNCHES"""
import csv
import json
import sys

trace, n = sys.argv[1], int(sys.argv[2])
rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
t = lambda r, k: int(r[k + "_Timestamp"]) / 1e3  # noqa: E731  (microseconds)
fused = [i for i, r in enumerate(rows) if "k_sim_fused" in r["Kernel_Name"]][-n:]
first, last = rows[fused[0]], rows[fused[-1]]
# the delivery kernels behind the last launch: everything that starts after it ends, up to the first
# gap of more than 1 ms (the bench's synchronize and what follows it)
tail, end = [], t(last, "End")
for r in rows[fused[-1] + 1:]:
    if t(r, "Start") - max(end, t(last, "End")) > 1000:
        break
    tail.append(r)
    end = max(end, t(r, "End"))
names = {}
for r in tail:
    k = r["Kernel_Name"].split("(")[0].split("::")[-1]
    names[k] = round(names.get(k, 0) + t(r, "End") - t(r, "Start"), 1)
print(json.dumps({
    "launches": len(fused),
    "launch_us": [round(t(rows[i], "End") - t(rows[i], "Start"), 1) for i in fused],
    "gap_us": [round(t(rows[b], "Start") - t(rows[a], "End"), 1) for a, b in zip(fused, fused[1:])],
    "first_start_to_last_end_us": round(t(last, "End") - t(first, "Start"), 1),
    "drain_us": round(end - t(last, "End"), 1),
    "timed_region_us": round(end - t(first, "Start"), 1),
    "drain_kernels_us": names,
}))
