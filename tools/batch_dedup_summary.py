"""Per-row verdict of an A/B of the batch calls from the raw outputs of
tools/find_many_rate.py, tools/collect_many_rate.py and
tools/find_k_many_rate.py (dev tool, no GPU): what wrote
profiles/batch_dedup/rates.jsonl.

usage: python tools/batch_dedup_summary.py RAW_DIR [LABEL ...] >> rates.jsonl

RAW_DIR holds one file per tool run, named LABEL.rRUN.TOOL.jsonl (TOOL =
find_many, collect_many or find_k_many; for profiles/host_dedup/ also find and
find_k, tools/find_rate.py and tools/find_k_rate.py): the stdout of that tree's
rate tool.
The labels `parent` and `parent2` are the parent commit's tree run twice (the
second gives the A/A spread on identical code); every other LABEL (default:
all found) is a tree under test.  A label is judged against the parent runs
of the runs it has itself.  Per tool row and label, one JSON line:
  parent / parent2 / LABEL   per run, the row's median ms of the batch call
                     (wall_median_ms; per request in part 1) and the library's
                     HIP-event kernel ms of the run's last round (one sample)
  aa_spread          |median(parent) - median(parent2)| / the smaller
  parent_range_widened  [min(parent) (1 - aa), max(parent) (1 + aa)]
  median, inside     LABEL's median of runs, and whether it lies in that range
  stats_equal        launches, fused, fallback, overflow, tasks_total, tasks,
                     total and max_answer equal in every run of all three
                     (tasks_run and records depend on dispatch order)
"""
import glob
import json
import os
import re
import statistics
import sys

KEY = ("part", "msg", "what", "target", "n", "k", "lo", "hi", "cap")
MEASURED = ("batch", "this", "find_many", "collect_many", "find_k_many", "find_k", "find")
STATS = ("launches", "fused", "fallback", "overflow", "tasks_total", "tasks", "total",
         "max_answer", "find_launches", "find_tasks_total", "answer", "answer_k")


def load(raw):
    """(tool, row key) -> label -> run -> (wall median ms, kernel ms, stats)."""
    rows = {}
    for f in sorted(glob.glob(os.path.join(raw, "*.r*.*.jsonl"))):
        m = re.fullmatch(r"(\w+)\.r(\d+)\.(\w+)\.jsonl", os.path.basename(f))
        if not m:
            continue
        label, run, tool = m.group(1), int(m.group(2)), m.group(3)
        for line in open(f):
            r = json.loads(line)
            if "part" not in r:
                continue
            key = tuple((k, r[k]) for k in KEY if k in r)
            wall = r[next(k for k in MEASURED if k in r)]["median_ms"]
            kms = next((r[k] for k in r if k.endswith("_kernel_ms") and not k.startswith("scan")),
                       None)
            stats = {k: r[k] for k in STATS if k in r}
            rows.setdefault((tool, key), {}).setdefault(label, {})[run] = (wall, kms, stats)
    return rows


def main():
    rows = load(sys.argv[1])
    want = sys.argv[2:]
    for (tool, key), by in sorted(rows.items(), key=lambda x: str(x[0])):
        for label in sorted(by):
            if label in ("parent", "parent2") or (want and label not in want):
                continue
            runs = sorted(r for r in by[label] if r in by["parent"] and r in by["parent2"])
            if not runs:
                continue
            rec = {"tool": f"tools/{tool}_rate.py", **dict(key), "label": label, "runs": runs}
            for lab in ("parent", "parent2", label):
                rec[lab] = {"wall_median_ms": [by[lab][r][0] for r in runs],
                            "kernel_ms_last_round": [by[lab][r][1] for r in runs]}
            rec["stats_equal"] = len({json.dumps(by[lab][r][2], sort_keys=True)
                                      for lab in ("parent", "parent2", label) for r in runs}) == 1
            p, p2, c = (statistics.median(rec[lab]["wall_median_ms"])
                        for lab in ("parent", "parent2", label))
            aa = abs(p - p2) / min(p, p2)
            lo = min(rec["parent"]["wall_median_ms"]) * (1 - aa)
            hi = max(rec["parent"]["wall_median_ms"]) * (1 + aa)
            rec.update(aa_spread=round(aa, 5), parent_range_widened=[round(lo, 5), round(hi, 5)],
                       median=round(c, 5), inside=lo <= c <= hi)
            print(json.dumps(rec))


if __name__ == "__main__":
    main()
