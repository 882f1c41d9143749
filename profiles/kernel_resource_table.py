"""Per-kernel resource table from a compiler log made with -Rpass-analysis=kernel-resource-usage:
python profiles/kernel_resource_table.py LOG [substring] -> one JSON object per kernel (VGPRs, AGPRs, spilled registers, scratch, LDS,
occupancy).  Used for the cotangent-form instances of the fused gradient kernel (profiles/vjp_timing.json)."""
import json
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def table(path, want=""):
    rows, cur = [], None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill", "TotalSGPRs": "sgprs",
            "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd",
            "LDS Size [bytes/block]": "lds_static_bytes"}
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = {"kernel": t.split(":", 1)[1].strip()}
            rows.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.rsplit(":", 1)
            if k.strip() in keys:
                cur[keys[k.strip()]] = int(v)
    names = demangle([r["kernel"] for r in rows])
    for r in rows:
        r["kernel"] = names.get(r["kernel"], r["kernel"])
    return [r for r in rows if want in r["kernel"]]


if __name__ == "__main__":
    for r in table(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""):
        print(json.dumps(r))
