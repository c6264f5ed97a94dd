"""Seeded per-episode domain randomisation on the GPU.

`wedm_draw_episode` is held to the host path of `sparc_amd.randomize` twice.  On raw guarded allocations (strides no
environment has, guard rows, poison in every column it must not touch) it is compared bit for bit with
`tests._episode_draw_ref.draw_columns`, which `tests/test_episode_sampler_host.py` holds to the host path in the same slot
groups and layouts; on real environments it is compared with the host path itself, on a twin on the CPU oracle backend that
follows the same calls -- bare draws, and ten control steps of the adapter with in-kernel autoreset on kernels 1 and 2."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from sparc_amd import EnvironmentConfig, EpisodeSampler, MaterialModuleParameters, WireEDMEnv, WireEDMVectorEnv, _abi, _lib
from sparc_amd.core import env_params as envp
from tests import _episode_draw_ref as ref
from tests import _geometry_ref as gref
from tests._compare import assert_blocks_equal
from tests.test_episode_sampler_host import (DEFAULTS, DIAMETERS, HEIGHT, MATERIALS, RANGES, SEED, WIRE, all_slots, assert_holds,
                                             masks, spec_of)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MP = MaterialModuleParameters()
CONSTS = {"base_flow_rate": 3.25, "dt_s": 1e-6}
N_SEG_MAX = 70  # of a 10 mm workpiece on WIRE's 0.2 mm grid with 2 mm buffers

# (slot group, layout, materials, diameters): layout "dynamic" derives the geometry rows, "static" selects them from the
# per-material table, "no material" has no material block (material 0), "params" nothing but the physics rows
CASES = [("params", "dynamic", 4, 3), ("damping", "dynamic", 4, 3), ("materials", "dynamic", 4, 3), ("geometry", "dynamic", 4, 3),
         ("height", "dynamic", 4, 3), ("all", "dynamic", 4, 3), ("all", "dynamic", 1, 1), ("all", "dynamic", 1, 3),
         ("all", "dynamic", 4, 1), ("materials", "static", 4, 0), ("materials", "static", 1, 0), ("geometry", "no material", 0, 3),
         ("params", "params", 0, 0)]
STRIDES = {1: (1, 64), 255: (255, 320), 256: (256, 259), 257: (257, 320)}


def kernel_masks(n):
    out = {"null": None, "zero": np.zeros(n, dtype=bool), "one": np.ones(n, dtype=bool), "alternating": np.arange(n) % 2 == 1}
    for lane in (255, 256):
        if lane < n:
            out[f"lane {lane}"] = np.arange(n) == lane
    return out


def descriptor(dev: dict, tables: dict, spec, layout, seed, offset, n, stride, materials, diameters, combo):
    """The `wedm_draw_desc` of a call on the device blocks `dev` (the blocks inside their guard rows)."""
    d = _abi.DrawDesc(seed=seed, env_id_offset=offset, num_envs=n, stride=stride, base_flow_rate=CONSTS["base_flow_rate"],
                      dt_s=CONSTS["dt_s"])
    for name, (lo, hi) in spec.get("params", {}).items():
        d.slot[envp.INDEX[name]] = _abi.DrawSlot(kind=_abi.DRAW_UNIFORM, lo=lo, hi=hi, span=hi - lo)
    if spec.get("materials"):
        d.slot[_abi.DRAW_SLOT_MATERIAL] = _abi.DrawSlot(kind=_abi.DRAW_CHOICE, k=spec["materials"])
    if spec.get("height") is not None:
        lo, hi = spec["height"]
        d.slot[_abi.DRAW_SLOT_HEIGHT] = _abi.DrawSlot(kind=_abi.DRAW_UNIFORM, lo=lo, hi=hi, span=hi - lo)
    if spec.get("diameters"):
        d.slot[_abi.DRAW_SLOT_DIAMETER] = _abi.DrawSlot(kind=_abi.DRAW_CHOICE, k=spec["diameters"])
    ptr = lambda name: dev[name].data_ptr()  # noqa: E731
    d.envp_src, d.envp_rows = ptr("envp_src"), ptr("envp_rows")
    if layout in ("dynamic", "static"):
        d.material_index, d.wmat_rows, d.wmat_table = ptr("mat_index"), ptr("wmat_rows"), tables["wmat_table"].data_ptr()
    if layout == "static":
        d.wmat_geom_table, d.geom_f64 = tables["wmat_geom_table"].data_ptr(), ptr("geom_f64")
    if layout in ("dynamic", "no material"):
        zs0, cb0 = gref.host_constants(WIRE)
        d.dynamic, d.height, d.diameter_index, d.geom_status = 1, ptr("height"), ptr("dia"), tables["status"].data_ptr()
        d.geom = _abi.GeomDeriveDesc(
            segment_len=WIRE.segment_len, buffer_len_bottom=WIRE.buffer_len_bottom, buffer_len_top=WIRE.buffer_len_top,
            contact_offset_top=WIRE.contact_offset_top, zone_start0=zs0, contact_bottom0=cb0, num_envs=n, n_seg_max=N_SEG_MAX,
            stride=stride, combo=tables["combo"].data_ptr(), n_diameters=diameters, n_materials=max(materials, 1),
            geom_f64=ptr("geom_f64"), geom_i32=ptr("geom_i32"))
    return d


def setup_call(n, stride, mask, case, seed=SEED, offset=0, rng_seed=5):
    """Guarded host allocations, their device copies, the descriptor and what the reference needs."""
    group, layout, materials, diameters = case
    _, spec = spec_of(group, materials, diameters)
    alloc, tables = ref.guarded_blocks(n, stride, max(materials, 1), max(diameters, 1), mask, np.random.default_rng(rng_seed), HEIGHT)
    if layout == "no material":
        del alloc["mat_index"]
    combo = None
    if layout in ("dynamic", "no material"):
        combo = gref.combination_table(MATERIALS[:max(materials, 1)], DIAMETERS[:diameters], WIRE, MP)
    dev_alloc = {name: torch.from_numpy(a.copy()).to(DEV) for name, a in alloc.items()}
    dev_tables = {name: torch.from_numpy(t).to(DEV) for name, t in tables.items()}
    dev_tables["status"] = torch.zeros(1, dtype=torch.int32, device=DEV)
    if combo is not None:
        dev_tables["combo"] = torch.from_numpy(np.ascontiguousarray(combo)).to(DEV)
    dev = {name: (a[1] if ref.SHAPES[name][0] is None else a[1:-1]) for name, a in dev_alloc.items()}
    desc = descriptor(dev, dev_tables, spec, layout, seed, offset, n, stride, materials, diameters, combo)
    geom = None if combo is None else {"wire": WIRE, "combo": combo, "n_diameters": diameters, "n_seg_max": N_SEG_MAX}
    t_mask = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    return alloc, tables, dev_alloc, dev_tables, dev, desc, spec, geom, t_mask


def launch(desc, t_mask, count):
    L = _lib.load()
    rc = L.wedm_draw_episode(C.byref(desc), None if t_mask is None else t_mask.data_ptr(), count.data_ptr(),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, (L.wedm_last_error(None) or b"").decode()


# ------------------------------------------------------------------------------------------------ 1: the kernel's memory
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_kernel_equals_the_reference_inside_guard_bands(n):
    """Every case on both strides of `n`, the masks and the two offsets rotating through them so that each occurs with each
    batch size; with all slots drawn, every mask.  Whole allocations are compared: guard rows, padding columns and unmasked
    columns hold 0xA5 before and after."""
    km = kernel_masks(n)
    names = list(km)
    runs = [(case, STRIDES[n][i % 2], names[(i + n) % len(names)], (0, 2 ** 31 + 5)[(i // 2) % 2]) for i, case in enumerate(CASES)]
    runs += [(CASES[5], STRIDES[n][1], name, 2 ** 31 + 5) for name in names]
    for case, stride, mask_name, offset in runs:
        mask = km[mask_name]
        alloc, tables, dev_alloc, dev_tables, dev, desc, spec, geom, t_mask = setup_call(n, stride, mask, case, offset=offset)
        for _ in range(2):  # the second draw reads what the first wrote (counts, source rows, stored geometry)
            rc, text = launch(desc, t_mask, dev["count"])
            assert rc == _abi.OK, (case, text)
            b = ref.inner(alloc)
            b.update(tables)
            assert ref.draw_columns(b, spec, SEED, offset, n, mask, CONSTS, geom) == 0
        torch.cuda.synchronize()
        assert int(dev_tables["status"].item()) == 0
        asked = np.ones(n, dtype=bool) if mask is None else mask
        keep = np.concatenate([~asked, np.ones(stride - n, dtype=bool)])
        for name, want in alloc.items():
            got = dev_alloc[name].cpu().numpy()
            assert got.tobytes() == want.tobytes(), (case, stride, mask_name, name, np.argwhere(got != want)[:4])
            assert ref.is_poison(got[[0, -1]]) and ref.is_poison(got[:, keep]), (case, stride, mask_name, name)
        for name, t in tables.items():
            assert dev_tables[name].cpu().numpy().tobytes() == t.tobytes(), name
        written = ref.inner(alloc)["count"][:n][asked]
        assert written.size == 0 or not ref.is_poison(written)


# ------------------------------------------------------------------------------------------------ 2: refusals
def test_refused_descriptors_write_nothing():
    n, stride = 100, 128
    alloc, tables, dev_alloc, dev_tables, dev, desc, spec, geom, t_mask = setup_call(n, stride, None, CASES[5])
    static = setup_call(n, stride, None, CASES[9])

    def changed(base, **fields):
        d = _abi.DrawDesc.from_buffer_copy(base)
        for key, value in fields.items():
            setattr(d, key, value)
        return d

    def slot(base, s, **fields):
        d = _abi.DrawDesc.from_buffer_copy(base)
        for key, value in fields.items():
            setattr(d.slot[s], key, value)
        return d

    def geom_field(base, **fields):
        d = _abi.DrawDesc.from_buffer_copy(base)
        for key, value in fields.items():
            setattr(d.geom, key, value)
        return d

    zeta, H, MAT, DIA = envp.INDEX["zeta"], _abi.DRAW_SLOT_HEIGHT, _abi.DRAW_SLOT_MATERIAL, _abi.DRAW_SLOT_DIAMETER
    count = dev["count"]
    bad = [
        (None, count, "null descriptor"), (desc, None, "draw_count"), (changed(desc, num_envs=0), count, "num_envs"),
        (changed(desc, stride=n - 1), count, "stride smaller"), (changed(desc, dynamic=2), count, "dynamic"),
        (slot(desc, zeta, lo=float("nan")), count, "finite"), (slot(desc, zeta, hi=float("inf")), count, "finite"),
        (slot(desc, zeta, span=float("inf")), count, "finite"), (slot(desc, zeta, lo=0.5, hi=0.25), count, "lo > hi"),
        (slot(desc, zeta, kind=_abi.DRAW_CHOICE, k=3), count, "kind"), (slot(desc, zeta, kind=7), count, "kind"),
        (slot(desc, MAT, k=0), count, "k >= 1"), (slot(desc, DIA, k=-1), count, "k >= 1"),
        (slot(desc, MAT, kind=_abi.DRAW_UNIFORM), count, "kind"),
        (slot(desc, MAT, k=3), count, "n_materials"), (slot(desc, DIA, k=4), count, "n_diameters"),
        (slot(desc, H, lo=0.0), count, "lo > 0"), (slot(desc, H, hi=10.5), count, "n_seg_max"),
        (changed(desc, envp_src=None), count, "envp_src"), (changed(desc, envp_rows=desc.envp_rows + 4), count, "envp_rows"),
        (changed(desc, material_index=None), count, "material_index"), (changed(desc, wmat_table=None), count, "wmat_table"),
        (changed(desc, height=None), count, "height"), (changed(desc, diameter_index=desc.diameter_index + 2), count, "diameter_index"),
        (changed(desc, dynamic=0), count, "wmat_geom_table"),
        (geom_field(desc, combo=None), count, "geom:"), (geom_field(desc, stride=stride + 64), count, "differs"),
        (geom_field(desc, n_seg_max=0), count, "geom:"),
        (changed(static[5], wmat_geom_table=None), static[4]["count"], "wmat_geom_table"),
        (slot(static[5], H, kind=_abi.DRAW_UNIFORM, lo=1.0, hi=2.0, span=1.0), static[4]["count"], "dynamic geometry only"),
    ]
    L = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for d, cnt, word in bad:
        cnt_ptr = None if cnt is None else cnt.data_ptr()
        rc = L.wedm_draw_episode(None if d is None else C.byref(d), None, cnt_ptr, stream)
        text = (L.wedm_last_error(None) or b"").decode()
        assert rc == _abi.ERR_BAD_ARG and text.startswith("wedm_draw_episode: ") and word in text, (word, rc, text)
    assert L.wedm_draw_episode(C.byref(desc), None, count.data_ptr() + 2, stream) == _abi.ERR_BAD_ARG  # a misaligned count array
    torch.cuda.synchronize()
    for host, device in ((alloc, dev_alloc), (static[0], static[2])):
        for name, want in host.items():
            assert device[name].cpu().numpy().tobytes() == want.tobytes(), name
    # the descriptors themselves are good: the same calls, unchanged, are accepted
    for d, cnt in ((desc, count), (static[5], static[4]["count"])):
        assert L.wedm_draw_episode(C.byref(d), None, cnt.data_ptr(), stream) == _abi.OK
    torch.cuda.synchronize()
    assert (dev["count"][:n].cpu().numpy() == ref.inner(alloc)["count"][:n] + 1).all()


# ------------------------------------------------------------------------------------------------ 3: kernel == host path
N = 100  # neither a multiple of 64 nor of 256


def make(device, n=N, materials=4, dynamic=True, offset=0, **kw):
    kw.setdefault("config", EnvironmentConfig(target_cutting_distance=5000.0))
    if device == "cpu":
        from tests._oracle_backend import OracleBackendRows

        kw["backend"] = OracleBackendRows
    if materials:
        kw["wire_material"] = [MATERIALS[k % materials] for k in range(n)]
        kw["wire_material_table"] = MATERIALS[:materials]
    if dynamic:
        kw["dynamic_geometry"] = {"max_workpiece_height": 10.0, "wire_diameters": DIAMETERS}
        kw["wire_diameter"] = np.resize(DIAMETERS, n)
    return WireEDMEnv(num_envs=n, device=device, wire_params=WIRE, env_id_offset=offset, env_params=dict(DEFAULTS),
                      workpiece_height=np.linspace(1.5, 9.5, n), **kw)


def sampler_blocks(env, s):
    n = env.num_envs
    out = {"count": s.draw_counts(), "envp_src": env._envp_src[:, :n], "envp_rows": env._envp_rows[:, :n],
           "geom_f64": env._geom_f64[:, :n], "geom_i32": env._geom_i32[:, :n]}
    if env._wmat_rows is not None:
        out.update(mat_index=env._wmat_index[:n], wmat_rows=env._wmat_rows[:, :n])
    if env._dyn is not None:
        out.update(height=env._dyn.height[:n], dia=env._dyn.dia[:n])
    return {k: v.cpu().clone() for k, v in out.items()}  # (a CPU tensor's .cpu() is the tensor itself: the twin steps on)


def assert_same_rows(gpu, sg, cpu, sc, what=None):
    a, b = sampler_blocks(gpu, sg), sampler_blocks(cpu, sc)
    for key in b:
        assert a[key].numpy().tobytes() == b[key].numpy().tobytes(), (what, key)


@pytest.mark.parametrize("layout", ["dynamic", "static", "no material"])
def test_environment_draws_equal_the_host_path(layout):
    """Bare draws on a real environment (257: two blocks, the second with one lane) and on its CPU twin: none, alternating,
    single and empty masks, one after the other, so that the counts differ between environments."""
    n = 257
    kw = {"dynamic": dict(), "static": dict(dynamic=False), "no material": dict(materials=0)}[layout]
    sk = dict(params=RANGES)
    if layout != "no material":
        sk["materials"] = True
    if layout != "static":
        sk.update(height=HEIGHT, diameters=True)
    gpu, cpu = make(DEV, n=n, offset=2 ** 31 + 5, **kw), make("cpu", n=n, offset=2 ** 31 + 5, **kw)
    sg, sc = EpisodeSampler(SEED, **sk), EpisodeSampler(SEED, **sk)
    for name in ("none", "alternating", "single", "zero", "alternating"):
        m = masks(n)[name]
        sg.draw(gpu, mask=None if m is None else torch.from_numpy(m).to(DEV), reset=False)
        sc.draw(cpu, mask=m, reset=False)
        assert_same_rows(gpu, sg, cpu, sc, name)
    gpu.check_errors()
    assert sg.draw_counts().max().item() == 4 and sg.draw_counts().min().item() == 1
    if layout == "dynamic":
        assert_holds(cpu, sc, sc.draw_counts().numpy() - 1)


# ------------------------------------------------------------------------------------------------ 4: the adapter, stepping
STEPS = 10
SHORT = EnvironmentConfig(target_cutting_distance=50.01)  # 10 nm past the initial gap: episodes of a few control steps
_TWIN = {}


def adapter(device):
    env = make(device, autoreset=True, reward="progress", config=SHORT, offset=3000)
    s = all_slots()
    return env, s, WireEDMVectorEnv(env, episode_sampler=s)


def twin_history():
    """The oracle twin's blocks after each control step, computed once."""
    if not _TWIN:
        env, s, vec = adapter("cpu")
        vec.reset(seed=12)
        act = env.make_action(0.5, 80.0, 9, 3.0, 30.0)
        hist = []
        for _ in range(STEPS):
            out = vec.step(act)
            hist.append((env.state.clone_blocks(), sampler_blocks(env, s), [t.clone() for t in out[:4]]))
        env.check_errors()
        _TWIN.update(hist=hist, counts=s.draw_counts().clone())
    return _TWIN


@pytest.mark.parametrize("kernel", [1, 2])
def test_adapter_equals_the_oracle_twin_after_every_control_step(kernel):
    t = twin_history()
    assert int(t["counts"].max()) >= 3 and int(t["counts"].min()) == 1, t["counts"]
    env, s, vec = adapter(DEV)
    env.set_kernel(kernel)
    vec.reset(seed=12)
    act = env.make_action(0.5, 80.0, 9, 3.0, 30.0)
    for i in range(STEPS):
        out = vec.step(act)
        blocks, rows, want = t["hist"][i]
        assert_blocks_equal(env.state.clone_blocks(), blocks, N)
        got = sampler_blocks(env, s)
        for key in rows:
            assert got[key].numpy().tobytes() == rows[key].numpy().tobytes(), (i, key)
        for a, b in zip(out[:4], want):
            assert torch.equal(a.cpu(), b), i
    name = env._backend.last_kernel()
    assert ("wedm_step_global" if kernel == 1 else "wedm_step_lanes_pk") in name, name
    env.check_errors()
    assert_holds_on_device(env, s)


def assert_holds_on_device(env, s):
    n = env.num_envs
    want = s.expected(env.env_id_offset + np.arange(n), s.draw_counts().cpu().numpy() - 1)
    got = {name: v.cpu().numpy() for name, v in env.get_env_params().items()}
    got["wire_material"] = env.get_wire_material_index().cpu().numpy()
    g = env.get_geometry()
    got.update(workpiece_height=g["workpiece_height"].cpu().numpy(), wire_diameter=g["wire_diameter"].cpu().numpy())
    for key, v in want.items():
        if key != "wire_diameter_index":
            assert got[key].tobytes() == v.astype(got[key].dtype).tobytes(), key


def test_adapter_steps_without_a_host_synchronisation():
    env, s, vec = adapter(DEV)
    vec.reset(seed=12)
    act = env.make_action(0.5, 80.0, 9, 3.0, 30.0)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(STEPS):
            vec.step(act)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    env.check_errors()
    assert torch.equal(s.draw_counts().cpu(), twin_history()["counts"])
    assert_holds_on_device(env, s)
