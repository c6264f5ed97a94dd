"""Checkpoint and resume of the whole training stack on the CPU oracle backends: a run that is
stopped at any control step, written through ``torch.save``, loaded with ``weights_only=True`` into fresh objects through
the public calls and continued hands out, and ends on, the bytes of the run that was never stopped.  Both sides are the same
code: there is no tolerance.  tests/test_resume.py runs the same functions on the MI355X."""
from __future__ import annotations

import pytest
import torch

from sparc_amd import Normalizer, WireEDMVectorEnv
from tests import _resume_common as rc
from tests._snapshot_common import make

DEV = "cpu"


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return tmp_path_factory.mktemp("resume-host")


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
    """What the public calls could do before the adapter had a `state_dict`: the dicts of the environment, the sampler and the
    normaliser.  If this did not differ from the uninterrupted run, the scenario would be too tame to test the property."""
    ref = rc.reference(variant, DEV, folder)
    differ = rc.control_differences(ref, variant, DEV)
    print(f"{variant}: without the adapter's own tensors the resume differs at cuts {sorted(differ)}")
    for k, what in differ.items():
        print(f"  cut {k}: {what}")
    partial = [k for k in rc.CUTS if 0 < int(ref["need"][k].sum()) < ref["need"][k].numel()]
    assert differ and set(differ) & set(partial), (differ, partial)


@pytest.mark.parametrize("which", ["all-s13", "all-s128", "dynamic"])
def test_an_environment_cut_in_mid_interval_continues_on_the_same_bytes(which, tmp_path):
    rc.check_mid_interval(which, DEV, tmp_path / "env.pt").close()


def test_every_mismatch_is_refused_before_a_byte_of_the_target_changes():
    rc.check_refusals(DEV)


def test_the_dict_holds_tensors_and_plain_values_and_names_what_it_leaves_out(tmp_path):
    vec = WireEDMVectorEnv(make(DEV, 6, "autoreset", "s13"), max_episode_steps=3000, wire_profile_bins=2, normalizer=Normalizer())
    vec.reset(seed=1)
    sd = vec.state_dict()
    assert set(sd) == {"num_envs", "autoreset", "max_episode_steps", "wire_profile_bins", "obs_names", "reward", "samplers",
                       "normalizer", "need_reset", "episode_count", "env"}
    assert sd["reward"] == "kernel" and sd["samplers"] == () and sd["obs_names"] == tuple(vec.obs_names)
    assert sd["need_reset"].device.type == "cpu" and sd["need_reset"].dtype == torch.bool and sd["episode_count"].dtype == torch.int64
    vec.save_checkpoint(tmp_path / "vec.pt")
    back = torch.load(tmp_path / "vec.pt", map_location="cpu", weights_only=True)
    assert back["obs_names"] == sd["obs_names"] and torch.equal(back["need_reset"], sd["need_reset"])
    vec.load_checkpoint(tmp_path / "vec.pt")
    assert "torch.Generator" in WireEDMVectorEnv.state_dict.__doc__ and "caller" in WireEDMVectorEnv.state_dict.__doc__
    vec.close()
