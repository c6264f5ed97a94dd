"""Checkpoint and resume of the whole training stack on the MI355X: the functions of
tests/_resume_common.py, which tests/test_resume_host.py runs on the CPU oracle backends, on ``cuda:0`` -- `wedm_step` with
and without the in-kernel reset, the masked `wedm_reset`, `wedm_draw_episode`, `wedm_normalize`, `wedm_gae`,
`wedm_policy_head` and `wedm_ppo_loss` in one loop that is cut at every control step, saved, loaded into fresh objects and
continued.  Both sides of every comparison but the last are the same code on the same device: there is no tolerance.  Nothing
is asserted about which instantiation a fresh handle's plan picks after a load (it has not yet seen a frozen lane and may pick
another): the results are promised to be the same."""
from __future__ import annotations

import pytest

from sparc_amd import _abi
from tests import _resume_common as rc
from tests._compare import assert_blocks_equal
from tests.test_episode_sampler import sampler_blocks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KERNEL = _abi.KERNEL
T_CUT = rc.T   # right after the first `finish`, before the epoch over that rollout


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return tmp_path_factory.mktemp("resume-gpu")


@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_the_uninterrupted_run_is_not_tame(variant, folder):
    rc.assert_honest(rc.reference(variant, DEV, folder), variant)


@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_a_resumed_stack_continues_on_the_bytes_of_the_uninterrupted_run(variant, folder):
    ref = rc.reference(variant, DEV, folder)
    for k in rc.CUTS:
        rc.check_resume(ref, variant, DEV, k)


@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_control_without_the_adapters_own_tensors_the_resume_differs(variant, folder):
    ref = rc.reference(variant, DEV, folder)
    differ = rc.control_differences(ref, variant, DEV)
    for k, what in differ.items():
        print(f"{variant}, cut {k}: {what}")
    partial = [k for k in rc.CUTS if 0 < int(ref["need"][k].sum()) < ref["need"][k].numel()]
    assert differ and set(differ) & set(partial), (differ, partial)


# (binding, forced kernel, lanes): the automatic plan and kernel 1 everywhere; the two-lane register kernel where the binding
# has a form of it (of the optional blocks it carries the pulse tally alone, and it takes uniform geometry only)
ALONE = [(which, 0, 0) for which in ("all-s13", "all-s128", "dynamic")] + \
        [(which, int(KERNEL.GLOBAL), 0) for which in ("all-s13", "all-s128", "dynamic")] + \
        [(which, int(KERNEL.REGS), 2) for which in ("pulse-s13", "pulse-s128")]


@pytest.mark.parametrize("which,kernel,lanes", ALONE, ids=[f"{w}-k{k}x{l}" for w, k, l in ALONE])
def test_an_environment_cut_in_mid_interval_continues_on_the_same_bytes(which, kernel, lanes, tmp_path):
    b = rc.check_mid_interval(which, DEV, tmp_path / "env.pt", kernel, lanes)
    try:
        ran = b._backend.last_form()
        if kernel:
            assert ran[0] == kernel and (not lanes or ran[1] == lanes), (ran, b._backend.last_kernel())
    finally:
        b.close()


def test_every_mismatch_is_refused_before_a_byte_of_the_target_changes():
    rc.check_refusals(DEV)


def test_the_resumed_run_on_the_device_equals_the_resumed_oracle_twin(folder):
    """The host-reset stack with the network evaluated on the host on both sides, cut between `finish` and the epoch: after
    the resume the device run ends on the twin's state blocks, sampler rows and rollout (`flat`), the blocks that the chain
    of oracle tests pins byte for byte."""
    variant, k = "host-reset", T_CUT
    ends = {}
    for dev in (DEV, "cpu"):
        ref = rc.reference(variant, dev, folder, net_device="cpu")
        st, _, _ = rc.resume(variant, dev, ref["paths"][k]["adapter"], net_device="cpu")
        try:
            rc.assert_equal(rc.everything(st), ref["end"], f"{variant} on {dev}, cut {k}")
            ends[dev] = (st.env.state.clone_blocks(), sampler_blocks(st.env, st.sampler), {n: v.detach().cpu().clone() for n, v in st.buf.flat().items()})
        finally:
            st.close()
    (blocks, rows, flat), (w_blocks, w_rows, w_flat) = ends[DEV], ends["cpu"]
    assert_blocks_equal(blocks, w_blocks, 70)
    rc.assert_equal(rows, w_rows, "sampler rows, device against twin")
    rc.assert_equal(flat, w_flat, "flat(), device against twin")

