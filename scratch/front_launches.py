"""usage: front_launches.py <dir with *kernel_trace.csv>: the launches between one replay's last kernel and the next replay's
encoder launch, late in the run, with start times relative to the previous replay's last kernel END; and the per-step mean of
the front's kernels over the run."""
import csv, glob, sys, collections
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
name = lambda r: r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")
enc = [i for i, r in enumerate(rows) if name(r).startswith("encoder_fused_kernel")]
FRONT = ("pack_nchw3", "stage_transition", "ef_src_fill", "step_front", "distribution", "normal", "uniform")
for k in (150, 180):
    a = enc[k]
    # walk back over the front's launches to the previous replay's last kernel
    i = a - 1
    while i > 0 and any(s in name(rows[i]) for s in FRONT):
        i -= 1
    t0 = int(rows[i]["End_Timestamp"])
    print(f"-- step {k}: us since the previous replay's last kernel ended (start, duration, queue, kernel)")
    for r in rows[i - 1:a + 2]:
        d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        print(f"{(int(r['Start_Timestamp']) - t0) / 1e3:9.1f} us  {d:7.1f}  q{r.get('Queue_Id', '?')}  {name(r)[:100]}")
tot, cnt = collections.Counter(), collections.Counter()
for r in rows:
    n = name(r)
    if any(s in n for s in FRONT) or n.startswith("encoder_fused_kernel"):
        tot[n[:80]] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        cnt[n[:80]] += 1
print("-- mean us per dispatch (dispatches)")
for n in tot:
    print(f"{tot[n] / cnt[n]:8.1f}  ({cnt[n]})  {n}")
