"""The captured train iteration without a device: the two entry points it adds to the C ABI (``cgs_adam_multi``, ``cgs_bn_moving_update``)
and the chunk plan of the multi-tensor Adam launch, which is a host function (``kernels.adam_chunk_plan``)."""
import ctypes
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cgs_adam_multi", "cgs_bn_moving_update")


def test_header_bindings_and_library_agree_on_the_new_entry_points():
    from cgs_amd import lib
    header = open(os.path.join(ROOT, "include", "cgs_hip.h")).read()
    declared = set(re.findall(r"\b(cgs_[a-z0-9_]+)\s*\(", header))
    l = lib.load()
    for name in NEW:
        assert name in declared and name in lib.SIGNATURES
        assert getattr(l, name) is not None
    # (table, n_slots, plan, n_chunks, lr_t, beta1, beta2, eps, stream): lr_t is a POINTER, the betas and eps stay values
    res, args = lib.SIGNATURES["cgs_adam_multi"]
    assert res is ctypes.c_int and len(args) == 9
    assert args[4] is ctypes.c_void_p and args[5:8] == [ctypes.c_float] * 3
    # (mean, invstd, moving_mean, moving_var, C, decay, eps, stream)
    res, args = lib.SIGNATURES["cgs_bn_moving_update"]
    assert res is ctypes.c_int and len(args) == 8 and args[:4] == [ctypes.c_void_p] * 4 and args[4] is ctypes.c_int
    for name in NEW:                                     # the header's argument lists are as long as the binding's
        decl = re.search(name + r"\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
        assert len(decl.split(",")) == len(lib.SIGNATURES[name][1]), (name, decl)
    assert l.cgs_version() >= 108


def test_the_slot_and_chunk_records_are_laid_out_as_the_header_declares_them():
    """kernels.AdamTable writes the two device arrays through numpy records: 5 x 8 bytes a slot, (int, unsigned, u64) a chunk."""
    header = open(os.path.join(ROOT, "include", "cgs_hip.h")).read()
    slot = re.search(r"typedef struct cgs_adam_slot \{(.*?)\}", header, re.S).group(1)
    chunk = re.search(r"typedef struct cgs_adam_chunk \{(.*?)\}", header, re.S).group(1)
    assert [f.split()[-1] for f in slot.strip().rstrip(";").split(";")] == ["w", "g", "m", "v", "n"]
    assert [f.strip() for f in chunk.strip().rstrip(";").split(";")] == ["int slot", "unsigned count", "unsigned long long begin"]


def check_plan(sizes, chunk):
    from cgs_amd.kernels import adam_chunk_plan
    plan = adam_chunk_plan(sizes, chunk)
    covered = [[0] * n for n in sizes]
    for slot, begin, count in plan:
        assert 0 <= slot < len(sizes)
        assert 1 <= count <= chunk and 0 <= begin and begin + count <= sizes[slot]        # never crosses (or leaves) its slot
        for i in range(begin, begin + count):
            covered[slot][i] += 1
    assert all(c == 1 for row in covered for c in row)                                     # every element exactly once
    assert len(plan) == sum((n + chunk - 1) // chunk for n in sizes)                       # the grid: no empty or split-short chunk
    assert all(slot != s for s, n in enumerate(sizes) if n == 0 for slot, _, _ in plan)    # an empty slot has no block
    assert [p[0] for p in plan] == sorted(p[0] for p in plan)
    return plan


@pytest.mark.parametrize("chunk", [1, 7, 256, 2048])
def test_chunk_plan_covers_every_element_of_every_slot_exactly_once(chunk):
    rng = random.Random(1000 + chunk)
    edges = [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1]
    check_plan([n for n in edges if n >= 0], chunk)
    check_plan([0], chunk)
    check_plan([], chunk)
    for _ in range(40):
        sizes = [rng.choice(edges + [rng.randrange(0, 6 * chunk + 2)]) for _ in range(rng.randrange(1, 12))]
        check_plan(sizes, chunk)


def test_chunk_plan_of_the_shipped_chunk_size():
    from cgs_amd import kernels as K
    assert K.ADAM_CHUNK == 2048
    plan = check_plan([1, 3, 255, 256, 257, 1025, 65537, 0], K.ADAM_CHUNK)
    assert len(plan) == 6 + 33 and plan[-1] == (6, 65536, 1)
    assert K.adam_chunk_plan([5000]) == [(0, 0, 2048), (0, 2048, 2048), (0, 4096, 904)]
    with pytest.raises(ValueError):
        K.adam_chunk_plan([4, -1])
    with pytest.raises(ValueError):
        K.adam_chunk_plan([4], 0)


def test_trainer_keeps_use_graph_off_by_default():
    import inspect
    from cgs_amd.training import GanTrainer
    assert inspect.signature(GanTrainer.__init__).parameters["use_graph"].default is False
