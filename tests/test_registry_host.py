"""The registry of step-kernel instantiations (sparc_amd/csrc/wedm_kernels.hip) seen through the library's debug seam
(wedm_debug_registry, wedm_debug_form_name), without a device: the Python mirrors of the kernel numbers and the form bits,
the registry's sanity, and the completeness of the catalogue that tests/test_registry_coverage.py runs on the GPU."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from sparc_amd import _abi, _lib
from tests import _registry_catalogue as cat

ROOT = Path(__file__).resolve().parents[1]
K, F = _abi.KERNEL, _abi.FORM


def _enum_body(text, opening):
    body = re.search(re.escape(opening) + r"\s*\{(.*?)\};", text, flags=re.S).group(1)
    return re.sub(r"//[^\n]*", "", body)


def test_form_bits_mirror_the_header_and_the_library_names_them_in_bit_order():
    """`_abi.FORM` equals the enum of F_* bits of wedm_device.h, and `wedm_debug_form_name(b)` -- the array `form_names()`
    spells its messages from -- names bit b as the enum does."""
    body = _enum_body((ROOT / "sparc_amd" / "csrc" / "wedm_device.h").read_text(), "enum : uint32_t")
    bits = {m.group(1): int(m.group(2)) for m in re.finditer(r"F_([A-Z0-9_]+)\s*=\s*1u\s*<<\s*(\d+)", body)}
    assert len(bits) == 14 and sorted(bits.values()) == list(range(14))
    assert {f.name: f.value for f in F} == {name: 1 << b for name, b in bits.items()}
    L = _lib.load()
    for name, b in bits.items():
        assert L.wedm_debug_form_name(b).decode() == name == F(1 << b).name
    for b in (-1, 14, 31, 32, 1000):
        assert L.wedm_debug_form_name(b) == b""


def test_kernel_numbers_mirror_the_kernel_unit():
    body = _enum_body((ROOT / "sparc_amd" / "csrc" / "wedm_kernels.hip").read_text(), "enum Kernel : int32_t")
    numbers = {m.group(1): int(m.group(2)) for m in re.finditer(r"K_([A-Z0-9_]+)\s*=\s*(\d+)", body)}
    assert len(numbers) == 13 and {k.name: k.value for k in K} == numbers


def test_registry_seam_reports_count_entries_and_bad_indices():
    L = _lib.load()
    k, lanes, forms = C.c_int32(), C.c_int32(), C.c_uint32()
    assert L.wedm_debug_registry(-1, C.byref(k), None, None) == _abi.OK
    count = k.value
    assert count == len(_lib.registry()) > 0
    for bad in (-2, count, count + 1, 2**31 - 1):
        assert L.wedm_debug_registry(bad, C.byref(k), C.byref(lanes), C.byref(forms)) == _abi.ERR_BAD_ARG
    assert L.wedm_debug_registry(-1, None, None, None) == _abi.ERR_BAD_ARG
    assert L.wedm_debug_registry(0, C.byref(k), None, C.byref(forms)) == _abi.ERR_BAD_ARG
    assert L.wedm_debug_last_form(None, C.byref(k), C.byref(lanes), C.byref(forms)) == _abi.ERR_BAD_ARG


def test_no_instantiation_is_registered_twice_and_every_family_has_one():
    """`find_instantiation` returns the first hit: a duplicate would be minutes of compile time for code that never runs."""
    reg = _lib.registry()
    seen, twice = set(), []
    for e in reg:
        if e in seen:
            twice.append(cat.describe(e))
        seen.add(e)
    assert not twice, twice
    assert {e[0] for e in reg} == {int(k) for k in K if k != K.AUTO}
    all_bits = sum(int(f) for f in F)
    for k, lanes, forms in reg:
        assert lanes in (0, 1, 2, 4, 8, 16) and not forms & ~all_bits, (k, lanes, forms)


def _readelf():
    for exe in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf"), shutil.which("llvm-readelf"),
                shutil.which("readelf")):
        if exe and os.path.exists(exe):
            return exe
    pytest.fail("no llvm-readelf / readelf to read the library's symbol table with")


def test_every_compiled_step_kernel_is_registered():
    """The registry's count equals the number of wedm_step_* kernels the library holds.  Counted from the library's symbol
    table (llvm-readelf of the ROCm toolchain, else binutils' readelf): hipcc emits one kernel handle, an 8-byte OBJECT
    symbol under the kernel's mangled name, per compiled __global__ instantiation.  (tools/kernel_resources.py --tsv lists
    the same kernels, but recompiles the whole library to do so: minutes, too long for a test.)"""
    out = subprocess.run([_readelf(), "--symbols", "--wide", str(_lib.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    handles = set()
    for line in out.splitlines():
        cols = line.split()
        if len(cols) >= 8 and cols[3] == "OBJECT" and re.match(r"_Z\d+wedm_step_", cols[7]):
            handles.add(cols[7])
    reg = _lib.registry()
    assert len(handles) == len(reg), (len(handles), len(reg))
    # and family by family: the mangled name starts with the family's name
    names = {1: "wedm_step_global", 2: "wedm_step_lanes_pk", 3: "wedm_step_fused", 4: "wedm_step_packed", 5: "wedm_step_split",
             6: "wedm_step_stream", 7: "wedm_step_regs", 8: "wedm_step_regs_wide", 9: "wedm_step_served", 10: "wedm_step_lanes",
             11: "wedm_step_lanes_served", 12: "wedm_step_regs_served"}
    for k, name in names.items():
        compiled = sum(1 for h in handles if re.match(rf"_Z{len(name)}{name}I", h))
        assert compiled == sum(1 for e in reg if e[0] == k), (name, compiled)


def test_every_registry_entry_has_a_recipe_or_is_listed_unreachable():
    """For every registered instantiation the catalogue names a (recipe, launch) expected to select it, or the entry is in
    UNREACHABLE with its reason; nothing the catalogue expects is missing from the registry; UNREACHABLE holds at most 8
    entries, none of them with a recipe."""
    reg = set(_lib.registry())
    assert len(cat.UNREACHABLE) <= cat.MAX_UNREACHABLE
    assert set(cat.UNREACHABLE) <= reg, "UNREACHABLE names an entry the registry does not hold"
    assert set(cat.CATALOGUE) == {int(k) for k in K if k != K.AUTO}
    expected = set()
    for k in cat.CATALOGUE:
        expected |= cat.expected_entries(k)
    assert all(reason.strip() for reason in cat.UNREACHABLE.values())
    assert not expected & set(cat.UNREACHABLE), [cat.describe(e) for e in expected & set(cat.UNREACHABLE)]
    without = sorted(reg - expected - set(cat.UNREACHABLE))
    assert not without, "no recipe and not UNREACHABLE: " + "; ".join(cat.describe(e) for e in without)
    unknown = sorted(expected - reg)
    assert not unknown, "the catalogue expects instantiations the registry does not hold: " + "; ".join(cat.describe(e) for e in unknown)


def test_recipes_are_distinct_and_their_launch_plans_hold_what_the_scenario_says():
    ids = [r.id for k in cat.CATALOGUE for r in cat.CATALOGUE[k]]
    assert len(ids) == len(set(ids))
    r = next(r for r in cat.CATALOGUE[int(K.FUSED)] if r.seq == "plain" and not r.bind and not r.autoreset)
    plan = r.launches()
    assert [us for us, *_ in plan] == [1, 1, 7, 290, 1, 7, 290]
    assert [sample for _, _, sample, _ in plan] == [False, False, False, False, False, True, True]
    for k in cat.CATALOGUE:
        for r in cat.CATALOGUE[k]:
            if r.n_envs != cat.N_ENVS:   # the batches of more than 65 536 lanes
                assert r.n_envs * r.lanes > cat.WIDE_AUTO_MAX_LANES >= (r.n_envs - 1) * r.lanes
                assert 9 <= r.n_seg <= 16 and sum(us for us, *_ in r.launches()) <= 20


def test_every_source_of_the_kernel_directory_is_built_and_hashed():
    """Every *.hip of csrc/ is the source of a build unit, and every file of csrc/ is among the sources the build id hashes
    and the build watches: a translation unit or a header added there cannot stay out of the library or of its fingerprint."""
    import __graft_entry__ as g

    csrc = ROOT / "sparc_amd" / "csrc"
    assert {src for src, _, _ in g.BUILD_UNITS} == set(csrc.glob("*.hip"))
    assert len({obj for _, _, obj in g.BUILD_UNITS}) == len(g.BUILD_UNITS)
    assert {f for f in csrc.iterdir() if f.is_file()} <= set(g.KERNEL_SOURCES)
