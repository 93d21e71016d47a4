"""Cascade attention without a device: the groups' bookkeeping (specdec.core.cascade.CascadeGroups), the plan query, the ABI
symbols and the refusals that come before device work (a model created over dummy pointers, as tests/test_kv_fp8_refusals_cpu.py)."""

import ctypes

import pytest

from specdec.core.cascade import CascadeGroups
from specdec_hip import _abi
from specdec_hip.ops import attention_cascade_plan, attention_plan
from test_kv_fp8_refusals_cpu import _model


def test_fork_chains_min_rule_and_floor():
    g = CascadeGroups(6)
    assert g.fork(1, 0, 1000) == 992 and g.flush() == [(0, 0, 992), (1, 0, 992)]        # floor to 32; the root carries the length
    assert g.fork(2, 1, 2000) == 992 and g.leader[2] == 0                               # through a member: min(c, shared_len(member))
    assert g.fork(3, 1, 500) == 480 and g.fork(4, 0, 2051) == 2048
    assert (g.leader, g.length) == ([0, 0, 0, 0, 0, 5], [2048, 992, 992, 480, 2048, 0])
    assert g.fork(5, 0, 31) == 0 and g.length[5] == 0                                   # below a block: stays out
    assert CascadeGroups(2, min_shared=1024).fork(1, 0, 1000) == 0
    assert g.stats() == (5, 992 + 992 + 480 + 2048)
    assert [e[0] for e in g.flush()][:1] == [0] and g.flush() == []                     # roots first; nothing changed since


def test_root_promotion_member_removal_and_dissolution():
    g = CascadeGroups(5)
    for b, c in ((2, 1024), (3, 512), (4, 2048)):
        g.fork(b, 1, c)
    g.flush()
    g.rewrite(1)                                   # the root's slot is rewritten: row 2 leads, the others keep min(own, row 2's)
    assert (g.leader, g.length) == ([0, 1, 2, 2, 2], [0, 0, 1024, 512, 1024])
    assert g.flush() == [(2, 2, 1024), (3, 2, 512), (4, 2, 1024), (1, 1, 0)]      # the old root leaves once nobody names it
    g.rewrite(4)                                   # a member leaves: the root's length follows its members
    assert g.length[2] == 512 and g.leader[4] == 4
    g.flush()
    g.rewrite(3)                                   # a group of one dissolves: the member's entry goes before its root's
    assert g.length == [0] * 5 and g.leader == list(range(5)) and g.flush() == [(3, 3, 0), (2, 2, 0)]
    g.fork(0, 1, 64)
    g.fork(0, 2, 64)                               # a forked slot leaves its old group first; that group was the two of them
    assert (g.leader, g.length) == ([2, 1, 2, 3, 4], [64, 0, 64, 0, 0])


def test_abi_plan_and_refusals_before_device_work():
    lib = _abi.load()
    assert lib.sd_abi_version() == 1
    for name in ("sd_model_set_cascade", "sd_model_set_shared_prefix", "sd_attention_cascade_plan"):
        assert hasattr(lib, name)
    p = attention_cascade_plan(24, 8, 128, 8, 5, 33024)            # 8 rows of the 3B geometry at K = 4: 120 stacked rows, 2 sets
    assert (p.tiles, p.n_split) == attention_plan(24, 8, 128, 8, 5, 33024)[:2] == (1, 8)
    assert (p.sets, p.p_split, p.slots, p.grid) == (2, 32, 8 * 8 * 40, (8, 8, 8 + 64))
    with pytest.raises(_abi.HipLibraryError, match="l_max % 32"):
        attention_cascade_plan(4, 2, 64, 1, 1, 1032)
    h, keep = _model(lib)
    assert lib.sd_model_set_shared_prefix(h, 0, 0, 0, None) != 0 and "sd_model_set_cascade" in _abi.last_error()
    assert lib.sd_model_set_cascade(h, 1) == 0
    assert lib.sd_model_set_kv_dtype(h, _abi.SD_FP8_E4M3, 1.0, 1.0) != 0 and "cascade" in _abi.last_error()
    assert lib.sd_model_set_shared_prefix(h, 0, 0, 0, None) != 0 and "not bound" in _abi.last_error()
    assert lib.sd_model_set_cascade(h, 0) == 0 and lib.sd_model_set_kv_dtype(h, _abi.SD_FP8_E4M3, 1.0, 1.0) == 0
    assert lib.sd_model_set_cascade(h, 1) != 0 and "fp8" in _abi.last_error()
    assert lib.sd_model_set_cascade(None, 1) != 0
    lib.sd_model_destroy(h)


def test_python_refusals_before_device_work():
    """the constructors refuse fp8 KV before they touch weights or the device; a session's refusals need no engine (check_session)"""
    import types

    from specdec.core import cascade
    from specdec.models.hip_lm import HipLM
    from specdec_hip.engine import HipModel

    with pytest.raises(ValueError, match="cascade_attention.*fp8"):
        HipModel(None, batch=1, l_max=64, kv_dtype="fp8", cascade=True)
    with pytest.raises(ValueError, match="cascade_attention.*fp8"):
        HipLM(None, kv_dtype="fp8", cascade_attention=True)
    pipe = types.SimpleNamespace(config={"draft_mode": "vanilla"}, _fake=False, medusa_heads=None, controller=types.SimpleNamespace(per_row=False),
                                 base_lm=types.SimpleNamespace(kv_cache_dtype="bf16"))
    cascade.check_session(pipe, True, False, False)
    for change, args, err, word in (({}, (False, False, False), ValueError, "share_prefix"), ({}, (True, True, False), NotImplementedError, "medusa"),
                                    ({}, (True, False, True), NotImplementedError, "context_window"),
                                    ({}, (True, False, False, False), NotImplementedError, "captured device step"),
                                    ({"_fake": True}, (True, False, False), NotImplementedError, "captured device step"),
                                    ({"controller": types.SimpleNamespace(per_row=True)}, (True, False, False), NotImplementedError, "adaptive K"),
                                    ({"base_lm": types.SimpleNamespace(kv_cache_dtype="fp8")}, (True, False, False), NotImplementedError, "fp8"),
                                    ({"config": {"draft_mode": "eagle"}}, (True, False, False), NotImplementedError, "eagle")):
        with pytest.raises(err, match=word):
            cascade.check_session(types.SimpleNamespace(**{**vars(pipe), **change}), *args)
    with pytest.raises(NotImplementedError, match="generate\\(\\)"):
        cascade.refuse_single(pipe, {"cascade_attention": True})
    assert not cascade.asked(pipe, None) and cascade.asked(pipe, True) and cascade.MIN_SHARED_DEFAULT == 32768
