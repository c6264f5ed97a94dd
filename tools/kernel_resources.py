#!/usr/bin/env python
"""Per-kernel register / scratch / LDS usage of the gfx950 build (hipcc -Rpass-analysis=kernel-resource-usage), compiled as
the build compiles it: the units of __graft_entry__.BUILD_UNITS, in parallel.

    python tools/kernel_resources.py [--tsv] [--out DIR] [extra hipcc flags...]

--tsv      one line per instantiation, tab-separated and sorted by name: the mangled name, the demangled name and the eight
           columns.  Nothing is truncated, so two builds compare with a plain `diff`.
--out DIR  keep the objects there, one directory per unit named after its object: DIR/wedm_kernels.part0 ... part5
           (with -save-temps=obj among the extra flags: the gfx950 assembly too)
"""
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g  # noqa: E402

args = sys.argv[1:]
tsv = "--tsv" in args
if tsv:
    args.remove("--tsv")
keep = "--out" in args
if keep:
    i = args.index("--out")
    out_dir = Path(args[i + 1]).resolve()
    out_dir.mkdir(parents=True, exist_ok=True)
    del args[i:i + 2]
else:
    out_dir = Path(tempfile.mkdtemp(prefix="wedm_resources_"))


def compile_unit(unit):
    d = out_dir / unit[2][:-len(".o")]  # a directory per unit: -save-temps names its files after the source
    d.mkdir(exist_ok=True)
    flags = [f for f in g.HIPCC_FLAGS if f != "-shared"] + ["-Rpass-analysis=kernel-resource-usage", *args]
    return g.start_unit(unit, d / unit[2], flags, "hipcc", stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)


procs = [compile_unit(unit) for unit in g.BUILD_UNITS]
rows, cur, failed = [], None, None
for p in procs:
    err = p.communicate()[1]
    if failed:
        continue
    if p.returncode != 0:
        failed = err
        for q in procs:  # the other parts have nothing left to tell
            if q.poll() is None:
                q.kill()
        continue
    for line in err.splitlines():
        m = re.search(r"remark:\s+(?:\S+:\d+:\d+:\s+)?(.*?) \[-Rpass", line)  # (-save-temps puts the location behind "remark:")
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = {"name": body.split(":", 1)[1].strip()}
            rows.append(cur)
        elif cur is not None and ":" in body:
            k, v = body.split(":", 1)
            cur[k.strip()] = v.strip()
if not keep:
    shutil.rmtree(out_dir, ignore_errors=True)
if failed:
    sys.exit(failed)
keys = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "Occupancy [waves/SIMD]",
        "LDS Size [bytes/block]"]
demangled = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.splitlines()
if tsv:
    print("\t".join(["mangled", "kernel", *keys]))
    for r, name in sorted(zip(rows, demangled), key=lambda rn: rn[0]["name"]):
        print("\t".join([r["name"], name, *(r.get(k, "-") for k in keys)]))
else:
    print(f"{'kernel':44s} " + " ".join(f"{k.split(' ')[0][:10]:>10s}" for k in keys))
    for r, name in zip(rows, demangled):
        print(f"{name[:44]:44s} " + " ".join(f"{r.get(k, '-'):>10s}" for k in keys))
