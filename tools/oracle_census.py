#!/usr/bin/env python
"""Branch census of the CPU oracle under the reference recordings.

Every GPU test compares a kernel with the oracle, and the oracle's only tie to the reference is the recordings under
tests/golden.  This tool answers which decisions of the oracle's per-microsecond step no recording has ever taken:
it builds oracle/wedm_oracle.c with gcc's coverage instrumentation (-O0, the Makefile's floating-point flags) in a
temporary directory, replays every fixture tests/test_oracle_golden.py names (same math modes) on that build in a
child process, runs `gcov -b` and prints the branches whose count is zero, identified by

    function name | stripped source text of the line | branch number

(no line numbers: they move with every edit).  A line whose text occurs more than once in a function carries `#2`,
`#3`... after the text.  tests/test_oracle_census.py holds the allowlist this output must equal.

    python tools/oracle_census.py            # one line per untaken branch
    python tools/oracle_census.py --json     # the same as a JSON list of [function, text, branch]
"""
from __future__ import annotations

import json
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SOURCE = ROOT / "oracle" / "wedm_oracle.c"
# the Makefile's flags with -O3 replaced by the instrumented -O0 (no inlining: every function keeps its own counters)
CFLAGS = ["--coverage", "-O0", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-std=gnu11"]

FUNCTIONS = (
    "debris_short_probability", "update_short_circuit_detection", "get_peak_current", "get_target_voltage",
    "get_on_time", "get_off_time", "get_lambda", "ignition_update", "material_update", "fast_exp", "dielectric_update",
    "update_convection_coefficients", "thermal_update_f32", "wire_update", "mechanics_update",
    "voltage_history_update", "wedm_oracle_step", "wedm_oracle_derive",
)


def replay_all(lib_path: str) -> int:
    """Child process: load the instrumented build in place of the oracle and replay the recordings.  The counters
    reach the .gcda file when the process exits."""
    sys.path.insert(0, str(ROOT))
    import ctypes as C

    import numpy as np

    from oracle import oracle as orc

    orc.LIB_PATH = Path(lib_path)  # before the first lib() call
    from tests import test_oracle_golden as tg
    from tests._golden import Fixture, action_for, replay

    golden = ROOT / "tests" / "golden"
    failed = []

    def run(name, **kw):
        fx = Fixture(golden / f"{name}.npz")
        bad, env = replay(fx, **kw)
        return fx, bad, env

    for name in list(tg.NATIVE) + list(tg.PHILOX):
        _, bad, _ = run(name, math_mode=orc.MATH_LIBM)
        if bad:
            failed.append((name, "LIBM", bad[:3]))
    for name in tg.PORTABLE:
        _, bad, _ = run(name, math_mode=orc.MATH_PORTABLE, exact_floats=False, float_rtol=1e-12, T_atol=1e-4)
        if bad:
            failed.append((name, "PORTABLE", bad[:3]))
    run("f1_config1_native", stencil_mode=orc.STENCIL_F64, exact_floats=False, float_rtol=1e-6, T_atol=1.3e-4,
        skip_floats=("tmax",))
    run("f2_single_spark")
    for name in tg.RAISING:  # the reference raised on the last step: replay() stops before it, the test takes it
        fx, _, env = run(name)
        orc.step(env, action_for(fx, fx.n_steps - 1))
    z = np.load(golden / "f4_geometry_table.npz")
    cols = json.loads(str(z["columns"]))
    for row in z["table"]:
        r = dict(zip(cols, row))
        cfg = orc.default_config(workpiece_height=r["h"], wire_diameter=r["d"], segment_len=r["seg"],
                                 buffer_len_bottom=r["buf_bottom"], buffer_len_top=r["buf_top"],
                                 contact_offset_bottom=r["off_bottom"], contact_offset_top=r["off_top"])
        orc.lib().wedm_oracle_derive(C.byref(cfg), C.byref(orc.Consts()))
    for f in failed:
        print("replay mismatch:", f, file=sys.stderr)
    return 1 if failed else 0


FUNC_RE = re.compile(r"^function (\S+) called (\d+)")
LINE_RE = re.compile(r"^\s*([0-9*#=-]+):\s*(\d+):(.*)$")
BRANCH_RE = re.compile(r"^branch\s+(\d+) (never executed|taken (\d+))")


def parse_gcov(text: str, functions=FUNCTIONS):
    """[(function, source text, branch number)] of the branches with a zero count inside `functions`."""
    untaken, func, line_text, seen = [], None, None, {}
    for raw in text.splitlines():
        m = FUNC_RE.match(raw)
        if m:
            func, line_text, seen = m.group(1), None, {}
            continue
        m = LINE_RE.match(raw)
        if m:
            if int(m.group(2)) == 0:
                continue
            body = " ".join(m.group(3).split())
            seen[body] = seen.get(body, 0) + 1
            line_text = body if seen[body] == 1 else f"{body} #{seen[body]}"
            continue
        m = BRANCH_RE.match(raw)
        if m and func in functions and line_text is not None:
            if m.group(2) == "never executed" or int(m.group(3)) == 0:
                untaken.append((func, line_text, int(m.group(1))))
    return untaken


def census():
    """Build, replay in a child process, gcov: the untaken branches of FUNCTIONS."""
    gcc, gcov = shutil.which("gcc"), shutil.which("gcov")
    if not gcc or not gcov:
        raise FileNotFoundError("gcc and gcov are needed for the census")
    with tempfile.TemporaryDirectory(prefix="wedm_census_") as tmp:
        so = str(Path(tmp) / "libwedm_oracle_census.so")
        subprocess.run([gcc, *CFLAGS, "-c", "-o", "wedm_oracle.o", str(SOURCE)], check=True, cwd=tmp)
        subprocess.run([gcc, "--coverage", "-fopenmp", "-shared", "-o", so, "wedm_oracle.o", "-lm"], check=True, cwd=tmp)
        subprocess.run([sys.executable, str(Path(__file__).resolve()), "--replay", so], check=True, cwd=tmp)
        out = subprocess.run([gcov, "-b", "-c", "--stdout", "-o", tmp, str(SOURCE)], check=True, cwd=tmp,
                             capture_output=True, text=True).stdout
    found = {m.group(1) for m in map(FUNC_RE.match, out.splitlines()) if m}
    missing = [f for f in FUNCTIONS if f not in found]
    if missing:
        raise RuntimeError(f"gcov reported no function named {missing}")
    return parse_gcov(out)


def main(argv):
    if len(argv) >= 2 and argv[0] == "--replay":
        return replay_all(argv[1])
    rows = census()
    if "--json" in argv:
        print(json.dumps(rows))
    else:
        for func, text, branch in rows:
            print(f"{func} | {text} | {branch}")
        print(f"{len(rows)} branches never taken", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
