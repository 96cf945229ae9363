"""usage: chain_launches.py DIR STEPS (DIR holds a rocprofv3 *kernel_trace.csv of a bench.py run of STEPS replays): per-step dispatch counts of the Q site's tail kernels and the ring wavefront's launch means"""
import csv, glob, sys, collections
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
steps = int(sys.argv[2])
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
name = lambda r: r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
cnt, tot = collections.Counter(), collections.Counter()
for r in rows:
    n = name(r).split("(")[0]
    cnt[n] += 1; tot[n] += dur(r)
for k in ("mlp_x_to_bf16_kernel", "mlp_wgrad_out_kernel", "mlp_wgrad_big_kernel", "mlp_wgrad_reduce_kernel", "mlp_wgrad_reduce_multi_kernel",
          "mlp_mid_fwd_kernel", "mlp_mid_bwd_kernel"):
    print(f"{k}: {cnt[k]} dispatches = {cnt[k] / steps:.2f} per step, mean {tot[k] / max(cnt[k], 1):.1f} us")
ring = [r for r in rows if "rnn_gemm_kernel" in name(r) and "<64, 64" not in name(r)]
per = 17
ring = ring[len(ring) % per:]
groups = [ring[i:i + per] for i in range(0, len(ring), per)][-150:]
first = sum(dur(g[0]) for g in groups) / len(groups)
third = sum(dur(g[2]) for g in groups) / len(groups)
total = sum(sum(dur(r) for r in g) for g in groups) / len(groups)
span = sum((int(g[-1]["End_Timestamp"]) - int(g[0]["Start_Timestamp"])) / 1e3 for g in groups) / len(groups)
print(f"ring wavefront over {len(groups)} steps: first launch {first:.1f} us, third launch {third:.1f} us, sum of 17 launches {total:.1f} us, first start to last end {span:.1f} us")
print("first-launch kernel:", name(groups[-1][0])[:60], "| second:", name(groups[-1][1])[:60])
