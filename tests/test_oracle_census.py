"""Which decisions of the oracle's per-microsecond step does no reference recording take?

Every GPU test compares a kernel with the CPU oracle, and the oracle is tied to the reference only through the
recordings under tests/golden: a decision no recording takes is a decision the oracle may restate wrongly with every
test green.  tools/oracle_census.py builds the oracle with branch counters, replays the recordings that
tests/test_oracle_golden.py replays and lists the branches that stayed at zero.  That list must equal the allowlist
below, in which every entry says why the REFERENCE cannot get there ("not recorded yet" is no reason: record it).
A new untaken branch therefore fails this test until it has a recording (tools/gen_golden.py) or a reason.

Not a sanitizer; nothing is preloaded.  Needs gcc's gcov (the compiler the oracle is built with ships it)."""
from __future__ import annotations

import json
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

VALIDATE = "EnvironmentConfig.validate() (core/env_config.py:73-90) raises for such a configuration: no environment, no recording"
OWN_LOG = "the crater-log ring is this project's own (the reference appends to a Python list); the single-environment replay binds none"
IN_RANGE = ("spark_y is drawn from [0, workpiece_height), so zone_start + y // segment_len lies in [zone_start, zone_end] "
            "and zone_end < n_seg with a top buffer of at least one segment: never negative, never past the wire")
SEG = "if (!(cfg->workpiece_height > 0) || !(cfg->wire_diameter > 0) || !(cfg->initial_gap > 0) ||"
SEG2 = "!(cfg->target_cutting_distance > 0) || cfg->dt <= 0 || cfg->servo_interval <= 0)"
LOG = "if (e->crater_log && e->crater_log_capacity > 0) /* crater_volumes_um3.append(sampled_volume_um3) :133 */"

# (function, stripped source text, gcov branch number) -> why the reference cannot take it
ALLOWED = {
    ("wedm_oracle_derive", SEG, 1): VALIDATE,
    ("wedm_oracle_derive", SEG, 3): VALIDATE,
    ("wedm_oracle_derive", SEG, 5): VALIDATE,
    ("wedm_oracle_derive", SEG2, 1): VALIDATE,
    ("wedm_oracle_derive", SEG2, 3): VALIDATE,
    ("wedm_oracle_derive", SEG2, 4): VALIDATE,
    ("wedm_oracle_derive", "if (n_seg > WEDM_ORACLE_MAX_SEG) return -2;", 0):
        "the oracle's own fixed capacity of 4096 cells; the reference allocates any length",
    ("wedm_oracle_derive", "o->joule_geom = (S != 0) ? delta_y / S : 0.0; /* :183 */", 1):
        "S = pi r^2 with wire_diameter > 0 by validate()",
    ("wedm_oracle_derive", "if (denominator == 0) return -3;", 0):
        "density * specific_heat * S * delta_y: positive material constants, S > 0, and a zero segment_len makes the "
        "reference's constructor divide by zero (wire.py:149) before any step",
    ("ignition_update", "} else if (s == -2) { /* _handle_rest_state :302-319 */", 1):
        "spark_status[0] only ever holds 0, 1, -1 or -2: the four handlers (ignition.py:247-319) assign nothing else",
    ("material_update", LOG, 0): OWN_LOG,
    ("material_update", LOG, 2): OWN_LOG,
    ("material_update", LOG, 3): OWN_LOG,
    ("material_update", "if (kerf > 0 && h > 0) {", 1):
        "kerf = base_overcut + wire_diameter + crater depth: wire_diameter > 0 by validate(), overcut and table depth are not negative",
    ("material_update", "if (kerf > 0 && h > 0) {", 3): "workpiece_height > 0 by validate()",
    ("dielectric_update", "if (e->cavity_volume > 0) {", 1):
        "cavity_volume = coeff * gap_mm with gap_um = max(0.001, d) >= 0.001 and coeff = pi * r_wire * workpiece_height > 0 by validate()",
    ("thermal_update_f32", "if (n > 1) {", 1):
        "n_seg = int((buffers + height) / segment_len) is 1 only for a segment longer than half the whole wire; the zone and both "
        "contacts then collapse onto cell 0, which is pinned to spool_T, and no reference run describes a wire",
    ("thermal_update_f32", "if (plasma_idx >= 0 && plasma_idx < n) dT[plasma_idx] = dT[plasma_idx] + (float)plasma_heat;", 3): IN_RANGE,
    ("thermal_update_f32", "float h = (i >= c->az_start && i < c->az_end && c->az_start < c->az_end) ? e->h_zone : e->h_base;", 5):
        "az_start <= i < az_end already implies az_start < az_end: the third test restates the slice's emptiness and cannot fail there",
    ("wire_update", "if (e->spark_state == 1 && !isnan(e->spark_y)) {", 3):
        "the ignition module writes state and location together (spark_status = [1, location, 0], ignition.py:264): a spark without a "
        "location does not exist",
    ("wire_update", ": c->zone_start;", 1): "segment_len == 0 makes the reference's constructor divide by zero (wire.py:149)",
    ("wire_update", "if (plasma_idx >= 0 && plasma_idx < c->n_seg) {", 1): IN_RANGE,
    ("wire_update", "if (plasma_idx >= 0 && plasma_idx < c->n_seg) {", 3): IN_RANGE,
    ("wire_update", "if (!isfinite(plasma_heat)) plasma_heat = 0.0;", 0):
        "plasma_heat = efficiency * voltage * current: a finite parameter, a latched finite voltage and a current from the table",
}

# the decisions the F19 recordings exist for (letters of the recordings' witnesses in tests/test_oracle_golden.py): never allowlisted
RECORDED = {
    "A": [("mechanics_update", "if (v > c->max_speed) v = c->max_speed;"), ("mechanics_update", "else if (v < -c->max_speed) v = -c->max_speed;")],
    "B": [("material_update", "if (!(sampled_um3 > 0)) sampled_um3 = 0; /* max(0, x) :130 */"), ("material_update", "if (crater_volume > 0) {"),
          ("dielectric_update", "if (crater > 0) e->debris_volume += crater;")],
    "C": [("dielectric_update", "e->debris_volume = nv > 0.0 ? nv : 0.0; /* max(0.0, nv) */")],
    "D": [("dielectric_update", "e->debris_density = q < 1.0 ? q : 1.0; /* min(1.0, q) */")],
    "E": [("debris_short_probability", "if (exponent > 500) return 0.0;"), ("debris_short_probability", "if (exponent < -500) return 1.0;")],
    "F": [("dielectric_update", "if (kd < 2.0) debris_factor = fast_exp(kd, e->math_mode);")],
    "G": [("update_convection_coefficients", "ve = ve > -0.9 ? ve : -0.9; /* max(-0.9, ve) */"),
          ("update_convection_coefficients", "h_base = floor_h > h_base ? floor_h : h_base; /* max(h_base, floor_h) */")],
    "H": [("get_peak_current", "if (m < 1 || m > WEDM_MAX_MODE) return e->c.default_current;"),
          ("material_update", "if (mode < 1 || mode > WEDM_MAX_MODE || !c->crater_valid[mode]) {")],
}


def test_allowlist_is_well_formed():
    source = " ".join((ROOT / "oracle" / "wedm_oracle.c").read_text().split())
    for (func, text, branch), reason in ALLOWED.items():
        assert len(reason) > 20 and "not yet" not in reason.lower(), (func, text)
        assert text in source, f"the allowlisted line of {func} is no longer in the oracle: {text}"
    lines = {(f, t) for f, t, _ in ALLOWED}
    for letter, decisions in RECORDED.items():
        for func, text in decisions:
            assert text in source, (letter, text)
            assert (func, text) not in lines, f"decision {letter} must be recorded, not allowlisted"


@pytest.mark.skipif(shutil.which("gcov") is None or shutil.which("gcc") is None, reason="gcov is not on the path")
def test_recordings_take_every_branch_of_the_step_but_the_allowlisted():
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "oracle_census.py"), "--json"], cwd=ROOT, check=True,
                         capture_output=True, text=True).stdout
    untaken = {(f, t, int(b)) for f, t, b in json.loads(out.strip().splitlines()[-1])}
    new = sorted(untaken - set(ALLOWED))
    gone = sorted(set(ALLOWED) - untaken)
    assert not new, "no recording under tests/golden takes these decisions of the oracle (record one, or say why none can):\n" + \
        "\n".join(f"  {f} | {t} | branch {b}" for f, t, b in new)
    assert not gone, "allowlisted as unreachable, yet taken (drop the entry):\n" + "\n".join(f"  {f} | {t} | branch {b}" for f, t, b in gone)
