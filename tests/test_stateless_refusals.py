"""The wording the five descriptor-taking training calls share, without a GPU: `wedm_normalize`, `wedm_gae`, `wedm_policy_head`,
`wedm_ppo_loss` and `wedm_episode_log` each refuse a null descriptor, a needed block that is NULL, the same block one byte off
its alignment and an output laid over an input -- and the three that work on tiles a tile range outside the workspace -- with
WEDM_ERR_BAD_ARG and exactly the text written out here.  The texts are the library's answers from before its entry points
shared their checks; every address is one nobody owns, so a call that launched would fail otherwise."""
from __future__ import annotations

import ctypes as C

import pytest

from sparc_amd import _abi, _lib

A = 0x100000  # the blocks lie 0x10000 apart: the largest below, 100 rows of 20 float32, has 8 000 bytes
LO, HI, LOG_SPAN = (-1.0, 0.0, 0.0, 0.0), (1.0, 200.0, 5.0, 100.0), (0.6931471805599453, 5.298317366548036, 1.6094379124341003,
                                                                      4.605170185988092)
TILES = "tile range outside the workspace: tile_offset + ceil(num_envs / 256) <= n_tiles_total <= 4096 must hold"


def at(*names):
    return {name: A + 0x10000 * i for i, name in enumerate(names)}


def norm_desc(**kw):
    f = dict(at("reward", "terminated", "truncated", "obs_out", "reward_out", "ret", "ep_return", "last_return", "ep_length",
                "last_length", "ep_count", "finished", "stats_in", "stats_out", "partials"),
             tile_offset=0, n_tiles_total=1, gamma=0.99, eps=1e-8, clip_obs=10.0, clip_reward=10.0,
             flags=_abi.NORM_UPDATE | _abi.NORM_STEP, num_envs=100)
    f.update(kw)
    d = _abi.NormDesc(**f)
    d.plane[0].rows, d.plane[0].n_rows, d.plane[0].stride = A + 0x100000, 8, 128
    return d


def gae_desc(**kw):
    f = dict(at("reward", "value", "last_value", "terminated", "truncated", "prev_done_in", "advantage", "returns",
                "advantage_norm", "valid", "prev_done_out", "partials", "moments"),
             in_stride=128, out_stride=128, gamma=0.99, lam=0.95, eps=1e-8, T=16, num_envs=100, tile_offset=0, n_tiles_total=1,
             flags=_abi.GAE_SKIP_AFTER_DONE | _abi.GAE_NORMALIZE)
    f.update(kw)
    return _abi.GaeDesc(**f)


def head_desc(**kw):
    f = dict(at("params", "u", "mode_index", "log_prob", "entropy"), param_stride=20, grad_stride=20, rows=100, n_modes=9,
             op=_abi.HEAD_EVALUATE)
    f.update(kw)
    d = _abi.HeadDesc(**f)
    d.lo[:], d.hi[:], d.log_span[:] = LO, HI, LOG_SPAN
    return d


def ppo_desc(**kw):
    f = dict(at("params", "value", "index", "u", "mode_index", "old_log_prob", "advantage", "returns", "old_value", "valid",
                "grad_params", "grad_value", "partials", "stats", "count"),
             param_stride=20, grad_stride=20, rows=100, n_src=150, clip=0.2, vf_coef=0.5, ent_coef=0.01, clip_value=0.2, n_modes=9,
             flags=_abi.PPO_CLIP_VALUE)
    f.update(kw)
    d = _abi.PpoDesc(**f)
    d.lo[:], d.hi[:], d.log_span[:] = LO, HI, LOG_SPAN
    return d


def elog_desc(dst=A + 0x110000, **kw):
    f = dict(at("terminated", "truncated", "mask", "env_out", "stamp_out", "head", "tile_counts"), capacity=64, stamp=1, n_planes=1,
             num_envs=100, tile_offset=0, n_tiles_total=1, flags=0)
    f.update(kw)
    d = _abi.ElogDesc(**f)
    q = d.plane[0]  # one plane of two float32 rows, summed
    q.src, q.dst, q.acc = A + 0x100000, dst, A + 0x120000
    q.src_stride, q.n_rows, q.elem_bytes, q.kind = 128, 2, 4, _abi.ELOG_SUM_F32
    return d


# export: (a descriptor that only a launch could stop, the needed block, the refusal of that block when it is NULL or one byte
# off, an output laid over an input (the statistics on one another, a block on a block's first or last element) and that
# refusal, whether the call has a tile range)
CALLS = {
    "wedm_normalize": (norm_desc, "partials", "partials is null or misaligned (UPDATE)",
                       dict(stats_out=A + 0xC0000), "stats_in and stats_out overlap", True),
    "wedm_gae": (gae_desc, "reward", "reward is null or not aligned to its element", dict(advantage=A), "advantage overlaps reward",
                 True),
    "wedm_policy_head": (head_desc, "params", "params is null or not aligned to its element", dict(log_prob=A + 7984),
                         "log_prob overlaps params", False),
    "wedm_ppo_loss": (ppo_desc, "params", "params is null or not aligned to its element", dict(partials=A),
                      "partials overlaps params", False),
    "wedm_episode_log": (elog_desc, "head", "head is null or not aligned to its element", dict(dst=A + 0x100000),
                         "plane 0.dst overlaps plane 0.src", True),
}


def answer(export, desc):
    L = _lib.load()
    rc = getattr(L, export)(None if desc is None else C.byref(desc), None)
    return rc, (L.wedm_last_error(None) or b"").decode()


@pytest.mark.parametrize("export", list(CALLS))
def test_the_shared_refusals_keep_their_code_and_their_text(export):
    make, block, unusable, overlap, overlapping, tiled = CALLS[export]
    assert answer(export, None) == (_abi.ERR_BAD_ARG, f"{export}: null descriptor")
    assert answer(export, make(**{block: None})) == (_abi.ERR_BAD_ARG, f"{export}: {unusable}")
    assert answer(export, make(**{block: getattr(make(), block) + 1})) == (_abi.ERR_BAD_ARG, f"{export}: {unusable}")
    assert answer(export, make(**overlap)) == (_abi.ERR_BAD_ARG, f"{export}: {overlapping}")
    if tiled:
        for outside in (dict(tile_offset=1), dict(tile_offset=-1), dict(n_tiles_total=0), dict(n_tiles_total=4097)):
            assert answer(export, make(**outside)) == (_abi.ERR_BAD_ARG, f"{export}: {TILES}")


def test_create_and_the_stateless_calls_write_one_text_per_thread():
    """`wedm_create` and the stateless entry points refuse into one thread-local text, whichever wrote last: a
    stateless refusal, `wedm_create`'s, a stateless refusal again, each read back through `wedm_last_error(NULL)` right after
    it; a thread that made no call reads an empty text.  `wedm_create` returns on its null check before any HIP call."""
    import threading

    L = _lib.load()
    texts = [answer("wedm_normalize", None)[1]]
    assert L.wedm_create(None, 1, 1, None) == _abi.ERR_BAD_ARG
    texts.append((L.wedm_last_error(None) or b"").decode())
    texts.append(answer("wedm_gae", None)[1])
    assert texts == ["wedm_normalize: null descriptor", "wedm_create: null pointer or non-positive size", "wedm_gae: null descriptor"]
    elsewhere = []
    t = threading.Thread(target=lambda: elsewhere.append(L.wedm_last_error(None)))
    t.start()
    t.join()
    assert elsewhere == [b""] and L.wedm_last_error(None) == b"wedm_gae: null descriptor"
