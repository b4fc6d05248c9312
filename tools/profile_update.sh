#!/bin/bash
# rocprofv3 evidence for the geometry refresh of a moving mesh (profiles/r06), run on an MI355X:
#   bash tools/profile_update.sh [output directory]        (default: prof_update_out/)
# tools/time_update.py un-profiled; then one --kernel-trace --stats run and, each on its own, a FETCH_SIZE and a WRITE_SIZE run of
# `tools/time_update.py hex216 --profile` (35 device-pointer updates of the 216^3 mesh).  Every step has its own time limit and a
# failed step ends the script.
set -u
OUT=${1:-prof_update_out}
mkdir -p $OUT
timeout -k 10 500 python3 tools/time_update.py hex216 del54 > $OUT/time_update.txt 2> $OUT/time_update.err
rc=$?; cat $OUT/time_update.txt; [ $rc -eq 0 ] || { tail -20 $OUT/time_update.err; echo "time_update failed ($rc)"; exit $rc; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -- python3 tools/time_update.py hex216 --profile > $OUT/stats.txt 2> $OUT/stats.err
rc=$?; [ $rc -eq 0 ] || { tail -20 $OUT/stats.err; echo "stats pass failed ($rc)"; exit $rc; }
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $OUT/pmc_$c -- python3 tools/time_update.py hex216 --profile > $OUT/pmc_$c.txt 2> $OUT/pmc_$c.err
  rc=$?; [ $rc -eq 0 ] || { tail -20 $OUT/pmc_$c.err; echo "pmc pass $c failed ($rc)"; exit $rc; }
done
python3 - "$OUT" <<'PY'
import collections, csv, glob, re, sys
out = sys.argv[1]
def short(k):
    k = k.replace("void ", "").replace("nin::(anonymous namespace)::", "")
    return re.split(r"[(<]", k)[0] + ("<true>" if "<true>" in k else "")
rows = list(csv.reader(open(glob.glob(out + "/stats/**/*kernel_stats.csv", recursive=True)[0])))
with open(out + "/kernel_stats.csv", "w", newline="") as f:
    csv.writer(f, quoting=csv.QUOTE_ALL).writerows(rows[:1] + [r for r in rows[1:] if "nin_update" in r[0] or "copyBuffer" in r[0]])
with open(out + "/pmc_summary.csv", "w", newline="") as f:
    w = csv.writer(f)
    w.writerow(["kernel", "counter", "dispatches", "mean_value_KiB", "mean_duration_us_under_pmc"])
    for c in ("FETCH_SIZE", "WRITE_SIZE"):
        acc, dur = collections.defaultdict(list), collections.defaultdict(list)
        for fn in glob.glob(out + f"/pmc_{c}/**/*counter_collection.csv", recursive=True):
            for r in csv.DictReader(open(fn)):
                k = short(r["Kernel_Name"])
                if r["Counter_Name"] == c and ("nin_update" in k or ("copyBuffer" in k and int(r["Grid_Size"]) > 100000)):
                    acc[k].append(float(r["Counter_Value"]))
                    dur[k].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        for k, v in acc.items():
            w.writerow([k, c, len(v), round(sum(v) / len(v), 1), round(sum(dur[k]) / len(dur[k]) / 1000, 1)])
print(open(out + "/kernel_stats.csv").read())
print(open(out + "/pmc_summary.csv").read())
PY
