#!/bin/bash
# HBM traffic of every kernel of a config-C frame (separate --pmc passes).
cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:?run this on the GPU box}"
out=gpurun_out/pmc_frame; mkdir -p $out
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $out/$c -o p -- python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-extras ${EXTRA_ARGS} > $out/$c.txt 2>&1 || { echo FAILED $c; tail -5 $out/$c.txt; exit 1; }
done
python - <<'PY'
import csv, glob, collections
res = {}
for c in ("FETCH_SIZE", "WRITE_SIZE"):
    f = glob.glob(f"gpurun_out/pmc_frame/{c}/*counter_collection.csv")[0]
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        agg[r["Kernel_Name"].split("(")[0][:48]].append(float(r["Counter_Value"]))
    res[c] = agg
import json
out = {}
for k in sorted(res["FETCH_SIZE"]):
    fv = res["FETCH_SIZE"][k]; wv = res["WRITE_SIZE"].get(k, [0])
    rd, wr = 2 * sum(fv) / len(fv) * 1024, sum(wv) / len(wv) * 1024     # FETCH_SIZE x2 (MI355X_MICROARCH.md), KB -> bytes
    out[k] = {"launches": len(fv), "read_bytes": round(rd), "write_bytes": round(wr)}
    print(f"{k:50s} launches={len(fv):4d}  read {rd/1e6:9.1f} MB  write {wr/1e6:9.1f} MB")
json.dump(out, open("gpurun_out/pmc_frame/traffic.json", "w"), indent=1)
PY
