"""The runs of profiles/tools/draft_step_ab.sh as profiles/draft_step_ab.txt: per script, row and timing column the ratio mean(2 branch runs) /
median(3 parent runs) and, in brackets, the spread (max - min) / median of the parent runs; > marks a ratio above 1 + spread."""
import glob, re, statistics, sys, os
scripts = ["k8v4_spec_bench", "k8v4_spec_wide_bench", "k8v4_layers_bench", "fp8_spec_window_bench", "fp8_spec_wide_bench", "mx4_spec_bench", "conn_host_time"]
def rows(path):
    out = {}
    for line in open(path):
        if "|" in line and ":" in line and not line.startswith("columns") and "clock" not in line:
            head, body = line.split(":", 1)
            vals = [float(seg.split()[0]) for seg in body.split("|") if re.match(r"\s*\d+\.\d+", seg)]
        else:
            m = re.match(r"\s*(.*?)\s+([\d.]+) (ms|us)\b", line)
            if not m:
                continue
            head, vals = m.group(1), [float(m.group(2))]
        if vals:
            out[" ".join(head.split())] = vals
    return out
lines, summary = [], []
for s in scripts:
    runs = {t: rows(os.path.join(os.environ.get("AB_OUT", "scratch/ab_runs"), f"{s}.{t}.txt")) for t in ("parent1", "branch1", "parent2", "branch2", "parent3")}
    worst, ws = [], []
    lines.append(f"{s}.py")
    for head, p1 in runs["parent1"].items():
        try:
            cols = []
            for c in range(len(p1)):
                p = [runs[t][head][c] for t in ("parent1", "parent2", "parent3")]
                b = [runs[t][head][c] for t in ("branch1", "branch2")]
                mp, mb = statistics.median(p), statistics.mean(b)
                sp = (max(p) - min(p)) / mp if mp else 0.0
                if not mp: continue
                cols.append((mb / mp, sp))
            worst.append(max(r - sp for r, sp in cols)); ws += cols
            lines.append(f"  {head:28s} " + " | ".join(f"{r:5.3f} ({sp:5.3f}){'>' if r > 1 + sp else ' '}" for r, sp in cols))
        except (KeyError, IndexError):
            lines.append(f"  {head}: not in every run")
    summary.append(f"{s}.py: ratios {min(r for r, _ in ws):.3f} .. {max(r for r, _ in ws):.3f}, median {statistics.median(r for r, _ in ws):.3f}; parent spreads {min(x for _, x in ws):.3f} .. {max(x for _, x in ws):.3f}; "
                   f"columns slower beyond their spread: {sum(r > 1 + x for r, x in ws)} of {len(ws)}")
print("\n".join(summary))
open("profiles/draft_step_ab.txt", "w").write("\n".join(summary + [""] + lines) + "\n")
