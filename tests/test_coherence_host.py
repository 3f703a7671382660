"""CPU: the decision "does the engine have to rebind or re-prepare?" of DynamicsWorldModel._bind, asked of a CPU model.

`world_model.bind_signature(model)` is what `_bind` compares with the signature of its last bind: it must change under every writer the
version counters or the module tree can show, stay put between two looks with nothing in between, and answer the same with and without
the memo of places (`engine_slots`) that the per-call path hands it.  A deep copy carries no engine state."""
import copy
import ctypes

import pytest
import torch

import coherence_cases as CC
from dreamer4_amd import world_model as WM


@pytest.fixture()
def model():
    return CC.dynamics()


def test_two_looks_with_nothing_in_between_agree(model):
    slots = WM.engine_slots(model)
    first = WM.bind_signature(model)
    assert first == WM.bind_signature(model) == WM.bind_signature(model, slots)
    names = [s[0] for s in first]
    assert len(set(names)) == len(names)
    bound = {k for k, _ in model.named_parameters()} | {k for k, _ in model.named_buffers()}
    assert set(names) <= bound and 'transformer.layers.0.3.fn.proj_out.weight' in names and 'register_tokens' in names
    assert not any(k in names for k in WM._NOT_BOUND)


@pytest.mark.parametrize('writer', sorted(CC.HOST_WRITERS))
def test_every_visible_writer_changes_the_signature(model, writer):
    slots = WM.engine_slots(model)                       # the memo of the per-call path, taken BEFORE the write; it keeps the old tensors alive
    before = WM.bind_signature(model, slots)
    CC.HOST_WRITERS[writer](model)
    after = WM.bind_signature(model, slots)
    assert after != before
    assert after == WM.bind_signature(model), 'the memo of places must not change the answer'
    assert after == WM.bind_signature(model, slots)


def test_a_swapped_parameter_shows_as_another_object_at_the_same_name(model):
    slots = WM.engine_slots(model)
    before = {s[0]: s for s in WM.bind_signature(model, slots)}
    old = CC.param(model, CC.SWAPPED_TRUNK)
    CC.w_swap_trunk(model)
    after = {s[0]: s for s in WM.bind_signature(model, slots)}
    assert old._version == before[CC.SWAPPED_TRUNK][4] and old.data_ptr() == before[CC.SWAPPED_TRUNK][2], 'the old object shows nothing'
    changed = [k for k in before if before[k] != after[k]]
    assert changed == [CC.SWAPPED_TRUNK]
    assert after[CC.SWAPPED_TRUNK][1] == id(CC.param(model, CC.SWAPPED_TRUNK)) != id(old)


def test_a_replaced_submodule_is_seen_through_the_memo(model):
    slots = WM.engine_slots(model)
    before = WM.bind_signature(model, slots)
    donor = CC.dynamics()
    model.transformer.layers._modules['0'] = donor.transformer.layers._modules['0']
    assert WM.bind_signature(model, slots) != before
    assert WM.bind_signature(model, slots) == WM.bind_signature(model)


def test_writes_to_the_heads_leave_the_signature_alone(model):
    """The heads are read through their pointers: a visible in-place write to them must not ask for a re-preparation of the trunk images
    (DreamTrainer steps them every iteration)."""
    before = WM.bind_signature(model)
    with torch.no_grad():
        for p in (*model.policy_head_parameters(), *model.value_head_parameters()):
            p.mul_(0.5)
    assert WM.bind_signature(model) == before


def test_the_invisible_write_is_invisible(model):
    """`.data` writes are the documented exception: nothing on the host can see them, `invalidate_prepared()` is the remedy."""
    before = WM.bind_signature(model)
    CC.param(model, CC.SCALED[1]).data.mul_(0.5)
    assert WM.bind_signature(model) == before
    slots = WM.engine_slots(model)
    model._bind_cache = (before, slots)                  # as _bind leaves it
    model.invalidate_prepared()
    forgotten, kept = model._bind_cache
    assert kept is slots and forgotten != WM.bind_signature(model, slots), 'the next call must not take the fast path'
    assert [e[:4] for e in forgotten] == [e[:4] for e in before], 'the bindings are kept: only the images are made again'


def test_mark_mutated_bumps_the_version_counters(model):
    from dreamer4_amd.optim import mark_mutated
    before = WM.bind_signature(model)
    w = CC.param(model, CC.SCALED[1])
    view, v0 = w.detach(), w._version
    mark_mutated([w])
    assert w._version == v0 + 1 and view._version == v0 + 1
    assert WM.bind_signature(model) != before


def test_a_deep_copy_carries_no_engine_state(model):
    model._engine, model._engine_caps = ctypes.c_void_p(0xdead0), (2, 16, 1, 0)           # faked: nothing is ever called with it
    model._ws = torch.zeros(8, dtype=torch.uint8)
    model._groups = dict(policy=dict(flat=torch.zeros(3)))
    model._bind_cache = (WM.bind_signature(model), WM.engine_slots(model))
    model._live_cache = WM.TimeCache(model, 2, 2, 7)
    model._cache_serial, model._engine_generation, model._slot_serial = 7, 3, [7, 7]
    try:
        twin = copy.deepcopy(model)
        fresh = type(model)._no_engine_state()
        for k, v in fresh.items():
            assert twin.__dict__[k] == v, k
        assert twin._engine is None and twin._ws is None and twin._bind_cache is None and twin._groups == {} and twin._live_cache is None
        assert model._engine.value == 0xdead0 and model._groups['policy']['flat'].numel() == 3, 'the original keeps its own'
        a, b = dict(model.named_parameters()), dict(twin.named_parameters())
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]) and (a[k].numel() == 0 or a[k].data_ptr() != b[k].data_ptr()), k
        assert {s[0] for s in WM.bind_signature(twin)} == {s[0] for s in WM.bind_signature(model)}
    finally:
        model._engine = None                              # (the destructor must not hand the faked handle to the library)
