#!/usr/bin/env python
"""Build an A/B variant of the HIP library with extra compiler flags (diagnostic; never the shipped library):

    python tools/build_variant.py W8 -DWEDM_STAGE_W=8      ->  build/ablate/libwedm_W8.so

The same parallel build of __graft_entry__.BUILD_UNITS as __graft_entry__.build_hip(); load it with WEDM_HIP_LIB=<path>
(tools/ab_*.sh alternate between the in-tree library and such variants on one box)."""
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g  # noqa: E402

tag, extra = sys.argv[1], sys.argv[2:]
# `--only-part UNIT`: compile that unit alone with the extra flags and take the other units' objects from the in-tree build
# (build/obj/) -- for switches that concern one kernel family only.  UNIT is a unit's object name without ".o"
# (wedm_kernels.part3) or, for a part of wedm_kernels.hip, its number alone (3 = the served kernels)
only = None
if "--only-part" in extra:
    i = extra.index("--only-part")
    names = {u[2][:-len(".o")]: u for u in g.BUILD_UNITS}
    only = names.get(extra[i + 1]) or names.get(f"wedm_kernels.part{extra[i + 1]}")
    if only is None:
        raise SystemExit(f"--only-part {extra[i + 1]}: no such build unit; the units are {', '.join(names)}")
    extra = extra[:i] + extra[i + 2:]
out = ROOT / "build" / "ablate" / f"libwedm_{tag}.so"
obj_dir = ROOT / "build" / "obj" / tag
obj_dir.mkdir(parents=True, exist_ok=True)
out.parent.mkdir(parents=True, exist_ok=True)
flags = [f for f in g.HIPCC_FLAGS if f != "-shared"] + ["-w", f'-DWEDM_BUILD_ID="{g.kernel_build_id()}+{tag}"'] + extra
procs, objs = [], []
for unit in g.BUILD_UNITS:
    if only is not None and unit != only:
        obj = ROOT / "build" / "obj" / unit[2]
        if not obj.exists():
            raise SystemExit(f"--only-part links the other units' objects from the in-tree build, and {obj} is missing: "
                             "build the library first (python __graft_entry__.py)")
        objs.append(obj)
        continue
    objs.append(obj_dir / unit[2])
    procs.append(g.start_unit(unit, objs[-1], flags))
if any(p.wait() != 0 for p in procs):
    raise SystemExit("compile failed")
subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(out), *map(str, objs)], check=True)
print(out)
